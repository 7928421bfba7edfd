// SSIMULACRA2 scorer for MI355X (gfx950): host side + the C ABI of include/ssimu2_hip.h.
//
// Replaces the one scorer call of oavif's target-quality search,
//   /root/reference/src/tq.zig:37  fssimu2.computeSsimu2(allocator, ref, dist, w, h, 3, null)
// (fssimu2 0.1.1 source is absent from the reference tree; the arithmetic follows the
// published SSIMULACRA2 v2.1 definition, see DESIGN.md "Oracle").
//
// Data layout in HBM, per ctx.  Every buffer is a DevBuf member of ssimu2_ctx, allocated by the first call that needs
// it and grouped there by the call that releases it ("Which call touches which buffer"):
//   frame       : ref and dist u8 frames, interleaved RGB8, w*h*3 bytes each (the reference's layout); the linear
//                 pyramids, scales 1..5 of both frames, planar fp32 linear RGB [3][h_s][w_s] (scale 0 is read straight
//                 from the u8 frames through the sRGB LUT); the fp64 [scale][18 stats][workgroups] partial sums
//   cache       : FIR mode, the cached reference: its positive-XYB planes and blur(ref*ref) planes, every scale
//   stage       : a decoded frame as uploaded (ssimu2_*_strided / _strided16)
//   rg          : SSIMU2_BLUR_RECURSIVE modes only (ssimu2_recursive.h), every scale packed: XYB planes of both frames,
//                 the reference's cached blur(x) / blur(x*x) planes, the horizontal pass of a pass's planes
//   map         : first map call only: density planes [scale][3][h_s][w_s] + the fp32 map [h][w] (ssimu2_error_map_*)
//   hbd, tab    : first 16-bit call only (ssimu2_*_rgb16 / _strided16): the u16 frames as uploaded and in the FIR mode
//                 their scale-0 linear planes [3][h][w]; the sRGB tables of depths 8..16
//   alpha       : first RGBA call only (the extension library's, ssimu2_ext.hip): the table of the 65,026 composite
//                 codes; the RGBA rows use `stage`, the composited u16 frames `hbd`
//   batch       : first batch call only (ssimu2_score_batch_*): staged frames, pyramids, partial sums and results of
//                 every item
//   result      : fp64 [108 averages][score][nscales], written by k_finalize straight into pinned host memory
//
// One score = ONE k_pyramid_bands launch (all five levels), ONE k_march launch covering all six scales, one
// k_finalize launch that writes its 880 bytes into the host mirror itself (recursive modes: conversion, horizontal
// pass, vertical pass + maps, k_finalize); everything on the ctx stream, no host sync inside (enqueue / wait
// split).  Streams the library creates are placed on distinct hardware queues ("stream placement").
#include <ctype.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <future>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>

#include "../../include/ssimu2_hip_internal.h"  // SSIMU2_MARCH_*
#define SSIMU2_CORE_UNIT 1  // the unit whose ssimu2_ctx the instrumented build may lay out differently
#include "ssimu2_host.h"    // ssimu2_ctx, DevBuf, launch, Feed: what this unit shares with the front ends
#include "ssimu2_kernels.h"
#include "ssimu2_recursive.h"

using namespace ssimu2;
using namespace ssimu2h;  // this unit defines every function ssimu2_host.h declares, each as ssimu2h::name

namespace {

constexpr uint32_t kMinLdsPerCu = 160u * 1024u;  // gfx950's; what ssimu2_ctx_create requires (include/ssimu2_hip.h)

const double kWeightsHost[108] = {
    0.0, 0.0007376606707406586, 0.0, 0.0, 0.0007793481682867309, 0.0,
    0.0, 0.0004371155730107379, 0.0, 1.1041726426657346, 0.00066284834129271,
    0.00015231632783718752, 0.0, 0.0016406437456599754, 0.0, 1.8422455520539298,
    11.441172603757666, 0.0, 0.0007989109436015163, 0.000176816438078653, 0.0,
    1.8787594979546387, 10.949069906051982, 0.0, 0.0007289346991508072,
    0.9677937080626833, 0.0, 0.00014003424285435884, 0.9981766977854967,
    0.00031949755934435053, 0.0004550992113792063, 0.0, 0.0, 0.0013648766163243398,
    0.0, 0.0, 0.0, 0.0, 0.0, 7.466890328078848, 0.0, 17.445833984131262,
    0.0006235601634041466, 0.0, 0.0, 6.683678146179332, 0.00037724407979611296,
    1.027889937768264, 225.20515300849274, 0.0, 0.0, 19.213238186143016,
    0.0011401524586618361, 0.001237755635509985, 176.39317598450694, 0.0, 0.0,
    24.43300999870476, 0.28520802612117757, 0.0004485436923833408, 0.0, 0.0, 0.0,
    34.77906344483772, 44.835625328877896, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
    0.0008680556573291698, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0005313191874358747, 0.0,
    0.00016533814161379112, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0004179171803251336,
    0.0017290828234722833, 0.0, 0.0020827005846636437, 0.0, 0.0, 8.826982764996862,
    23.19243343998926, 0.0, 95.1080498811086, 0.9863978034400682, 0.9834382792465353,
    0.0012286405048278493, 171.2667255897307, 0.9807858872435379, 0.0, 0.0, 0.0,
    0.0005130064588990679, 0.0, 0.00010854057858411537};

// FIR taps of the sigma = 1.5 recursive Gaussian (Charalampidis 2016 truncated cosines,
// N = 5): w(d) = sum_k n2_k / sin(w_k) * sin(w_k (d + N)); see DESIGN.md "Blur".
void gaussian_taps(double sigma, float taps[5], float n2_out[3], float d1_out[3]) {
    const double kPi = 3.141592653589793238;
    const double radius = round(3.2795 * sigma + 0.2546);
    const double pi_div_2r = kPi / (2.0 * radius);
    const double om[3] = {pi_div_2r, 3.0 * pi_div_2r, 5.0 * pi_div_2r};
    const double p1 = 1.0 / tan(0.5 * om[0]), p3 = -1.0 / tan(0.5 * om[1]),
                 p5 = 1.0 / tan(0.5 * om[2]);
    const double r1 = p1 * p1 / sin(om[0]), r3 = -p3 * p3 / sin(om[1]),
                 r5 = p5 * p5 / sin(om[2]);
    double rho[3];
    for (int i = 0; i < 3; ++i) rho[i] = exp(-0.5 * sigma * sigma * om[i] * om[i]) / radius;
    const double D13 = p1 * r3 - r1 * p3, D35 = p3 * r5 - r3 * p5, D51 = p5 * r1 - r5 * p1;
    const double z15 = D35 / D13, z35 = D51 / D13;
    // solve [p1 p3 p5; r1 r3 r5; z15 z35 1] beta = gamma by Cramer's rule
    const double g[3] = {1.0, radius * radius - sigma * sigma,
                         z15 * rho[0] + z35 * rho[1] + rho[2]};
    const double a = p1, b = p3, c = p5, d = r1, e = r3, f = r5, gg = z15, hh = z35, ii = 1.0;
    const double det = a * (e * ii - f * hh) - b * (d * ii - f * gg) + c * (d * hh - e * gg);
    const double beta0 = (g[0] * (e * ii - f * hh) - b * (g[1] * ii - f * g[2]) +
                          c * (g[1] * hh - e * g[2])) / det;
    const double beta1 = (a * (g[1] * ii - f * g[2]) - g[0] * (d * ii - f * gg) +
                          c * (d * g[2] - g[1] * gg)) / det;
    const double beta2 = (a * (e * g[2] - g[1] * hh) - b * (d * g[2] - g[1] * gg) +
                          g[0] * (d * hh - e * gg)) / det;
    const double beta[3] = {beta0, beta1, beta2};
    for (int t = 0; t < 5; ++t) {
        double wsum = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double n2 = -beta[k] * cos(om[k] * (radius + 1.0));
            wsum += n2 / sin(om[k]) * sin(om[k] * (t + radius));
        }
        taps[t] = (float)wsum;
    }
    // the recursion itself (SSIMU2_BLUR_RECURSIVE): input gain and feedback of each section
    for (int k = 0; k < 3; ++k) {
        n2_out[k] = (float)(-beta[k] * cos(om[k] * (radius + 1.0)));
        d1_out[k] = (float)(-2.0 * cos(om[k]));
    }
}

thread_local std::string g_create_error;

// Instrumented build: record whether hbd.lin0_ref / hbd.lin0_dist hold the w x h scale-0 planes of the last score or
// reference (1: they do from now on, 0: they do not, -1: unchanged).  Nothing in the product library.
inline void note_lin0(ssimu2_ctx* c, int ref, int dist, uint32_t w, uint32_t h) {
#ifdef SSIMU2_INSTRUMENTED_BUILD
    if (ref >= 0) {
        c->lin0_ref_w = ref ? w : 0;
        c->lin0_ref_h = ref ? h : 0;
    }
    if (dist >= 0) {
        c->lin0_dist_w = dist ? w : 0;
        c->lin0_dist_h = dist ? h : 0;
    }
#else
    (void)c, (void)ref, (void)dist, (void)w, (void)h;
#endif
}

// Instrumented build: which marching kernel the score or batch being enqueued launches (SSIMU2_MARCH_* of
// include/ssimu2_hip_internal.h, 0 = none).  Nothing in the product library.
inline void note_march(ssimu2_ctx* c, int kind) {
#ifdef SSIMU2_INSTRUMENTED_BUILD
    c->last_march = kind;
#else
    (void)c, (void)kind;
#endif
}

struct Pyramid {
    int w[kNumScales], h[kNumScales];
    size_t lin_off[kNumScales];  // float offset of scale s (s >= 1) in the lin buffers
    size_t lin_total;
    int nscales;
};

// Scale s is scored iff scale s-1 is at least 8x8 (the published loop tests the size
// before downsampling).
Pyramid make_pyramid(uint32_t w, uint32_t h) {
    Pyramid p{};
    int cw = (int)w, ch = (int)h;
    size_t off = 0;
    p.nscales = 0;
    for (int s = 0; s < kNumScales; ++s) {
        if (cw < 8 || ch < 8) break;
        if (s) {
            cw = (cw + 1) / 2;
            ch = (ch + 1) / 2;
            p.lin_off[s] = off;
            off += (size_t)3 * cw * ch;
        }
        p.w[s] = cw;
        p.h[s] = ch;
        ++p.nscales;
    }
    p.lin_total = off;
    return p;
}

// Rows per workgroup (segment length) of the marching kernel.  A segment of R rows costs R + 8
// rows of conversion and horizontal blur, so longer is cheaper; shorter gives more workgroups
// to balance.  Measured on MI355X at 4K (scripts/gpu_sweep2.sh): the full-resolution scale is
// best at ~512 workgroups (two thirds of the 768 resident slots, 6 % halo), the smaller scales
// at ~48 rows -- their few, long workgroups overlap the tail of scale 0 and, with two
// streams, the next score.  Bounds: >= 8 rows, <= 160 rows (fp32 partial sums per lane).
// kSegRuleCols is the rule's own column unit, not a kernel's strip width: the rows a lane sums in fp32 are part of a
// score's bits (tests/gpu_cases.py restates the rule), so they stay what they were when the strips became wider.
constexpr int kSegRuleCols = 120;
int march_seg_rule(const Pyramid& p, int scale) {
    const int nstrips = (p.w[0] + kSegRuleCols - 1) / kSegRuleCols;
    int nsegs = (512 + nstrips / 2) / nstrips;
    if (nsegs < 1) nsegs = 1;
    int seg = (p.h[0] + nsegs - 1) / nsegs;  // full-resolution scale: ~512 workgroups
    if (seg < 8) seg = 8;
    if (seg > 160) seg = 160;
    // smaller scales: 48 rows, but never longer than the full-resolution segments, or their
    // workgroups would outlast scale 0's on small frames
    if (scale > 0 && seg > 48) seg = 48;
    return seg;
}

int march_seg_rows(const ssimu2_ctx* c, const Pyramid& p, int scale) {
    if (scale > 0 && c->seg_rows_tail_override > 0) return c->seg_rows_tail_override;
    if (scale == 0 && c->seg_rows_override > 0) return c->seg_rows_override;
    return march_seg_rule(p, scale);
}

// Segment rows of a BATCH item (ssimu2_score_batch_*): a function of the frame size and the scale ONLY -- never of
// the number of items or of an item's place among them -- so that an item's score is a property of its pair and not
// of the batch it travelled in.  A batch does not need scale 0 cut into ~512 workgroups to fill the GPU (the other
// items do that), so its segments are long: kBatchSegRows rows at scale 0 (a workgroup converts and blurs R + 8 rows
// for R rows scored), at most 48 below it as in a single score.  The choice among the single-score rule and 48, 96
// and 160 fixed rows is measured: scripts/gpu_batch_bench.py, profiles/batch_score.json, DESIGN.md section 11.
constexpr int kBatchSegRows = 96;
int batch_seg_rows(const ssimu2_ctx* c, const Pyramid& p, int scale) {
    int seg = c->batch_seg_override > 0 ? c->batch_seg_override
              : c->batch_seg_override < 0 ? march_seg_rule(p, 0) : kBatchSegRows;
    if (scale > 0 && seg > 48) seg = 48;
    return seg;
}

using SegRows = int (*)(const ssimu2_ctx*, const Pyramid&, int);

// Output columns per strip of the marching kernel a plan is built for -- the one place that knows which entry point
// has which geometry (ssimu2_kernels.h, MarchGeo): the kernels that leave partial sums (pair, cached reference, 16-bit,
// batch) march wide strips, the ones that write planes (k_ref_blur, the map kernels) narrow ones.
enum MarchOut { MARCH_OUT_SUMS, MARCH_OUT_PLANES };
constexpr int strip_cols(MarchOut out) { return out == MARCH_OUT_SUMS ? MarchWide::MW : MarchNarrow::MW; }

// What the final reduction needs of the frame size alone; `part` and `nblocks` are the caller's.
FinalizeArgs finalize_args(const Pyramid& p) {
    FinalizeArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.nscales = p.nscales;
    for (int s = 0; s < p.nscales; ++s) fa.inv_pixels[s] = 1.0 / ((double)p.w[s] * (double)p.h[s]);
    return fa;
}

// float offset of scale s in a plane set of every scale (the cached reference's XYB and blur planes; scale 0 first)
size_t xyb_off(const Pyramid& p, int s) {
    size_t off = 0;
    for (int k = 0; k < s; ++k) off += (size_t)3 * p.w[k] * p.h[k];
    return off;
}

// Where a marching plan reads and writes: what build_plans turns into the per-scale pointers.
struct PlanSources {
    const void *ref0, *dist0;         // scale 0 of the two frames: 8-bit frames, or linear planes (the *_lin kernels)
    const float *lin_ref, *lin_dist;  // their linear pyramids: scale s >= 1 at Pyramid::lin_off[s]
    const float* ref_xyb;             // null, or plane sets with scale s at xyb_off(p, s): the reference's positive XYB
    float* ref_s11;                   // and blur(ref*ref) (k_ref_blur, k_march_map: the planes the kernel writes)
    double* part;                     // partial sums of one pair; null: sizes only, the plans' pointers stay null
};

// A marching plan and its final reduction under a segment-rows rule (march_seg_rows or batch_seg_rows).  The one place
// for the sizes -- per scale w, h, segment rows, strips, workgroups and their running total, 1 / pixels -- and the one
// place that writes the per-scale pointers, from `src`.  Returns the workgroups of one pair's marching launch (none
// for a frame below 8 x 8), each with kStats doubles of partial sums.  `out`: what the kernel that will run the plan
// leaves behind, which fixes its strip width (strip_cols).
int build_plans(const ssimu2_ctx* c, const Pyramid& p, SegRows seg_rows, const PlanSources& src, MarchPlan* mp,
                FinalizeArgs* fa, MarchOut out = MARCH_OUT_SUMS) {
    memset(mp, 0, sizeof *mp);
    *fa = finalize_args(p);
    mp->nscales = p.nscales;
    int blocks = 0;
    for (int s = 0; s < p.nscales; ++s) {
        const int seg = seg_rows(c, p, s);
        const int nstrips = (p.w[s] + strip_cols(out) - 1) / strip_cols(out);
        const int nb = nstrips * ((p.h[s] + seg - 1) / seg);
        mp->blk_end[s] = blocks + nb;
        mp->w[s] = p.w[s];
        mp->h[s] = p.h[s];
        mp->seg[s] = seg;
        mp->nstrips[s] = nstrips;
        mp->nblocks[s] = fa->nblocks[s] = nb;
        if (src.part) {
            mp->ref[s] = s == 0 ? src.ref0 : (const void*)(src.lin_ref + p.lin_off[s]);
            mp->dist[s] = s == 0 ? src.dist0 : (const void*)(src.lin_dist + p.lin_off[s]);
            mp->ref_xyb[s] = src.ref_xyb ? src.ref_xyb + xyb_off(p, s) : nullptr;
            mp->ref_s11[s] = src.ref_s11 ? src.ref_s11 + xyb_off(p, s) : nullptr;
            fa->part[s] = mp->part[s] = src.part + (size_t)blocks * kStats;
        }
        blocks += nb;
    }
    return blocks;
}

// ---- the buffers: one grow, one release ---------------------------------------------------------
bool fits(const DevBuf& b, size_t bytes) { return b.p && bytes <= b.cap; }

// `b` holds at least `bytes` afterwards: grown on demand, never shrunk, the old content is not kept.  The stream is
// drained before the old block is freed.  Any failure leaves `b` released; a failed allocation is SSIMU2_ERR_OOM with
// `what` and leaves no sticky HIP error behind.
int grow(ssimu2_ctx* c, DevBuf& b, size_t bytes, const char* what) {
    if (fits(b, bytes)) return SSIMU2_OK;
    hipError_t e = hipStreamSynchronize(c->stream);
    b.release();
    if (e != hipSuccess) return c->fail(SSIMU2_ERR_HIP, "hipStreamSynchronize(c->stream)", e);
    e = b.host ? hipHostMalloc(&b.p, bytes, hipHostMallocDefault) : hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return c->fail(SSIMU2_ERR_OOM, what, e);
    }
    b.cap = bytes;
    return SSIMU2_OK;
}

// Release every buffer of a group (a struct of DevBuf members, or one DevBuf).
template <class G>
void release(G& group) {
    static_assert(std::is_standard_layout<G>::value && sizeof(G) % sizeof(DevBuf) == 0, "a group holds DevBufs only");
    for (DevBuf* b = (DevBuf*)&group; b != (DevBuf*)(&group + 1); ++b) b->release();
}

void release_recursive(ssimu2_ctx* c) {
    release(c->rg);
    (void)hipFree(c->d_rg_q);
    c->d_rg_q = nullptr;
}

// Everything sized by the frame or holding content of the frame buffers: every group except the batch scratch, the
// 16-bit tables and the result -- and with them the reference they held.  The caller has drained the stream.
void release_frame_groups(ssimu2_ctx* c) {
    c->ref.drop();
    release(c->frame);
    release(c->cache);
    release(c->stage);
    release_recursive(c);
    release(c->map);
    release(c->hbd);
}

// The u8 frames, linear pyramids and partial sums for a w x h frame: all five or none.  Each grows to max(need,
// current); growing any of them releases every group release_frame_groups names and drops the reference.  On failure
// everything is released.
int ensure_capacity(ssimu2_ctx* c, uint32_t w, uint32_t h) {
    const Pyramid p = make_pyramid(w, h);
    MarchPlan mp;
    FinalizeArgs fa;
    const size_t need_u8 = (size_t)w * h * 3, need_lin = (p.lin_total + 4) * sizeof(float),
                 need_part = ((size_t)build_plans(c, p, march_seg_rows, {}, &mp, &fa) * kStats + 8) * sizeof(double);
    struct {
        DevBuf& b;
        size_t bytes;
    } want[5] = {{c->frame.ref_u8, need_u8}, {c->frame.dist_u8, need_u8}, {c->frame.lin_ref, need_lin},
                 {c->frame.lin_dist, need_lin}, {c->frame.partials, need_part}};
    bool ok = true;
    for (auto& x : want) {
        ok = ok && fits(x.b, x.bytes);
        if (x.bytes < x.b.cap) x.bytes = x.b.cap;
    }
    if (ok) return SSIMU2_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    release_frame_groups(c);
    for (auto& x : want) {
        const int rc = grow(c, x.b, x.bytes, "hipMalloc(frame buffers)");
        if (rc) {
            release_frame_groups(c);
            return rc;
        }
    }
    return SSIMU2_OK;
}

// Band-pyramid arguments of up to two frames: levels 1..nscales-1 of frames[i] into lin[i].
PyrBandArgs pyramid_args(const Pyramid& p, int nframes, const uint8_t* const* frames, float* const* lin) {
    PyrBandArgs a{};
    a.nlevels = p.nscales > 1 ? p.nscales - 1 : 0;
    for (int l = 0; l < p.nscales; ++l) {
        a.w[l] = p.w[l];
        a.h[l] = p.h[l];
        a.opitch[l] = p.w[l];  // tight rows (the linear-light pyramid); rg_launch_convert pads them
    }
    a.nframes = nframes;
    a.bands_x = (p.w[0] + PYR_BAND_W - 1) / PYR_BAND_W;
    a.bands_y = (p.h[0] + PYR_BAND_H - 1) / PYR_BAND_H;
    for (int f = 0; f < nframes; ++f) {
        a.in[f] = frames[f];
        for (int l = 0; l < a.nlevels; ++l) a.out[f][l] = lin[f] ? lin[f] + p.lin_off[l + 1] : nullptr;
    }
    return a;
}

// Linear-light pyramids of up to two frames as a launch of their own (all levels, one launch).
void launch_pyramid(ssimu2_ctx* c, const Pyramid& p, int nframes, const uint8_t* const* frames,
                    float* const* lin) {
    if (p.nscales < 2) return;
    const PyrBandArgs a = pyramid_args(p, nframes, frames, lin);
    launch(k_pyramid_bands, dim3(a.bands_x * a.bands_y * nframes), dim3(PYR_THREADS), 0, c->stream, a);
}

// ---- 16-bit input (Src16: ssimu2_host.h) ------------------------------------
PyrHbdArgs hbd_args(int nframes, const Src16* const* src, float* const* lin0) {
    PyrHbdArgs hb{};
    for (int f = 0; f < nframes; ++f) {
        hb.in[f] = (const uint8_t*)src[f]->px;
        hb.pitch[f] = src[f]->pitch;
        hb.tab[f] = src[f]->tab;
        hb.maxv[f] = src[f]->maxv;
        hb.lin0[f] = lin0 ? lin0[f] : nullptr;
    }
    return hb;
}

// FIR: levels 1..nscales-1 of up to two 16-bit frames (same channel count) into lin[i], their scale-0 linear planes
// into lin0[i].  Launched for any frame with a scale: the marching kernel reads scale 0 from lin0.
void launch_pyramid16(ssimu2_ctx* c, const Pyramid& p, int nframes, const Src16* const* src, float* const* lin,
                      float* const* lin0) {
    if (p.nscales < 1) return;
    const uint8_t* none[2] = {nullptr, nullptr};
    const PyrBandArgs a = pyramid_args(p, nframes, none, lin);
    const PyrHbdArgs hb = hbd_args(nframes, src, lin0);
    launch(src[0]->ch == 4 ? k_pyramid_bands16<4> : k_pyramid_bands16<3>, dim3(a.bands_x * a.bands_y * nframes),
           dim3(PYR_THREADS), 0, c->stream, a, hb);
}

// The reference's cached planes, both sets (FIR mode): what the refblur kernels and every 16-bit pass need.
bool ref_cached(const ssimu2_ctx* c) { return c->cache.xyb.p && c->cache.blur.p; }

// A single score on the context's own buffers: scale 0 from ref0 / dist0, the scales below from its linear pyramids,
// with `ref_xyb_cached` the reference's cached planes as far as they exist.  Other sources: change the field.
PlanSources score_sources(const ssimu2_ctx* c, const void* ref0, const void* dist0, bool ref_xyb_cached) {
    return {ref0, dist0, c->frame.lin_ref.as<float>(), c->frame.lin_dist.as<float>(),
            ref_xyb_cached ? c->cache.xyb.as<float>() : nullptr,
            ref_xyb_cached && ref_cached(c) ? c->cache.blur.as<float>() : nullptr, c->frame.partials.as<double>()};
}

// The marching launch of a score or (`batch`: the plan around `mp`) a batch, chosen from three facts: the reference's
// blur is cached, scale 0 is linear planes (16-bit input), this is a batch.  Launches only if there are workgroups.
void launch_march(ssimu2_ctx* c, bool cached, bool lin0, const MarchPlan& mp, const MarchBatchPlan* batch = nullptr) {
    const int blocks = mp.nscales > 0 ? (batch ? batch->blk_end : mp.blk_end)[mp.nscales - 1] : 0;
    note_march(c, blocks <= 0 ? SSIMU2_MARCH_NONE
                  : batch     ? (cached ? SSIMU2_MARCH_REFBLUR_BATCH : SSIMU2_MARCH_PAIR_BATCH)
                  : lin0      ? (cached ? SSIMU2_MARCH_REFBLUR_LIN : SSIMU2_MARCH_PAIR_LIN)
                              : (cached ? SSIMU2_MARCH_REFBLUR_U8 : SSIMU2_MARCH_PAIR_U8));
    if (blocks <= 0) return;
    const dim3 grid((unsigned)blocks), threads(MARCH_THREADS);
    if (batch) launch(cached ? k_march_refblur_batch : k_march_batch, grid, threads, 0, c->stream, *batch);
    else if (lin0) launch(cached ? k_march_refblur_lin : k_march_lin, grid, threads, 0, c->stream, mp);
    else launch(cached ? k_march_refblur : k_march, grid, threads, 0, c->stream, mp);
}

// Positive-XYB planes of one frame at every scale into the plane set `xyb` (scale s at xyb_off(p, s)): scale 0 from
// `scale0` (`scale0_u8`: an 8-bit frame, else linear planes), the scales below from the linear pyramid `lin`.
void launch_ref_xyb(ssimu2_ctx* c, const Pyramid& p, const void* scale0, bool scale0_u8, const float* lin, float* xyb) {
    for (int sc = 0; sc < p.nscales; ++sc)
        launch(k_ref_xyb, dim3((unsigned)(((size_t)p.w[sc] * p.h[sc] + 255) / 256)), dim3(256), 0, c->stream,
               sc == 0 ? scale0 : (const void*)(lin + p.lin_off[sc]), sc == 0 && scale0_u8, p.w[sc], p.h[sc],
               xyb + xyb_off(p, sc));
}

// ---- the published-recursion modes (ssimu2_recursive.h) ------------------------------------------
// plane offset (floats per plane) of scale s in the packed recursive-mode buffers
size_t rg_plane_off(const Pyramid& p, int s) {
    size_t off = 0;
    for (int k = 0; k < s; ++k) off += (size_t)rg_pitch(p.w[k]) * p.h[k];  // rows padded to 128 floats ("Row pitch")
    return off;
}

constexpr uint64_t kRgMaxPixels = 1ull << 28;  // 21 planes of 1.33 n floats: 30 GB at this size

int rg_check_size(ssimu2_ctx* c, uint32_t w, uint32_t h) {
    if ((uint64_t)w * h > kRgMaxPixels)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "recursive blur mode: image larger than 2^28 pixels");
    return SSIMU2_OK;
}

// Scratch + cache of the recursive modes for this frame size.  The planes and their partial sums are replaced
// together when either is too small, which drops a cached reference (its planes live here); a failure leaves both
// released.  The debug planes follow rg_dbg_scale.
int rg_ensure(ssimu2_ctx* c, const Pyramid& p) {
    const size_t ntot = rg_plane_off(p, p.nscales);
    const size_t need = (21 * ntot + (size_t)rg_pitch(p.w[0]) + 16) * sizeof(float);  // + the dump row of k_rg_v_emit
    size_t need_part = 8 * sizeof(double);
    for (int s = 0; s < p.nscales; ++s) need_part += (size_t)kStats * ((p.w[s] + RG_VW - 1) / RG_VW) * sizeof(double);
    const char* what = "hipMalloc(recursive-blur planes: 84 bytes per pixel and scale)";
    if (!fits(c->rg.planes, need) || !fits(c->rg.part, need_part)) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->rg.planes.release();
        c->rg.part.release();
        c->ref.drop();
        int rc;
        if ((rc = grow(c, c->rg.planes, need, what)) || (rc = grow(c, c->rg.part, need_part, what))) {
            c->rg.planes.release();
            return rc;
        }
    }
    if (!c->d_rg_q) {
        HIP_TRY(c, hipMalloc(&c->d_rg_q, 4 * sizeof(unsigned)));
        c->num_cus = c->dev.compute_units > 0 ? (int)c->dev.compute_units : 256;
    }
    if (c->rg_dbg_scale >= 0 && c->rg_dbg_scale < p.nscales) {  // 15 h planes + 9 v planes
        const size_t nd = (size_t)24 * rg_pitch(p.w[c->rg_dbg_scale]) * p.h[c->rg_dbg_scale] + 16;
        return grow(c, c->rg.dbg, nd * sizeof(float), "hipMalloc(recursive-blur debug planes)");
    }
    return SSIMU2_OK;
}

// A recursive-mode plan of one w x h frame: every field that follows from the frame size (the pointers stay null), and
// where its buffers lie -- the 21 planes of `planes` ([xa 3][xb 3][cache 6][hbuf 9], each with every scale packed, as
// the context's rg.planes and a pair-form batch item have them) and the partial sums `part`.  One pair's workgroups of
// the horizontal pass, of the vertical pass, and its doubles of partial sums are what it returns.
struct RgCounts {
    int hblocks, vblocks;
    size_t part;
};
RgCounts rg_plan_geometry(const Pyramid& p, RgPlan* rp) {
    memset(rp, 0, sizeof *rp);
    rp->nscales = p.nscales;
    RgCounts n{0, 0, 0};
    for (int s = 0; s < p.nscales; ++s) {
        rp->w[s] = p.w[s];
        rp->h[s] = p.h[s];
        rp->pitch[s] = rg_pitch(p.w[s]);
        rp->vgroups[s] = (p.w[s] + RG_VW - 1) / RG_VW;
        rp->hblk_end[s] = n.hblocks += 3 * ((p.h[s] + RG_HL - 1) / RG_HL);
        rp->vblk_end[s] = n.vblocks += 3 * rp->vgroups[s];
        n.part += (size_t)kStats * rp->vgroups[s];
    }
    rp->vjobs = n.vblocks;  // jobs of the persistent vertical pass: one channel of 64 columns, largest scale first
    return n;
}
void rg_plan_buffers(const Pyramid& p, RgPlan* rp, float* xa, float* xb, float* cache, float* hbuf, double* part) {
    for (int s = 0; s < p.nscales; ++s) {
        const size_t off = rg_plane_off(p, s);
        rp->xa[s] = xa + 3 * off;
        rp->xb[s] = xb + 3 * off;
        rp->cache[s] = cache + 6 * off;
        rp->hbuf[s] = hbuf + 9 * off;
        rp->part[s] = part;
        part += (size_t)kStats * rp->vgroups[s];
    }
}

// Plan of one frame's share of a recursive-mode score: `ref_frame` selects where the frame's XYB
// planes go (xa, the reference's, or xb).
void rg_build_plan(const ssimu2_ctx* c, const Pyramid& p, bool ref_frame, RgPlan* rp, int* hblocks, int* vblocks) {
    const RgCounts n = rg_plan_geometry(p, rp);
    const size_t ntot = rg_plane_off(p, p.nscales);
    float* xa = c->rg.planes.as<float>();
    float* xb = xa + 3 * ntot;
    float* cache = xb + 3 * ntot;
    float* hbuf = cache + 6 * ntot;
    rg_plan_buffers(p, rp, xa, xb, cache, hbuf, c->rg.part.as<double>());
    for (int s = 0; s < p.nscales; ++s) rp->xout[s] = (ref_frame ? xa : xb) + 3 * rg_plane_off(p, s);
    rp->dump = hbuf + 9 * ntot;
    rp->q = c->d_rg_q;
    *hblocks = n.hblocks;
    *vblocks = n.vblocks;
}

// Instrumented builds (ssimu2_instr_rg_stop_after_scale): keep the raw planes of one scale for the
// parity tests.  After a horizontal pass its planes are copied out of hbuf; the per-pass planes of
// the vertical pass exist only in LDS, so k_rg_v_emit recomputes them into the debug buffer.
bool rg_debugging(const ssimu2_ctx* c, const Pyramid& p) {
    return c->rg.dbg.p && c->rg_dbg_scale >= 0 && c->rg_dbg_scale < p.nscales;
}

void rg_debug_keep_h(ssimu2_ctx* c, const Pyramid& p, const RgPlan& rp, bool ref) {
    const int s = c->rg_dbg_scale, nk = ref ? 2 : 3;
    const size_t n = (size_t)rg_pitch(p.w[s]) * p.h[s];
    for (int ch = 0; ch < 3; ++ch)
        for (int k = 0; k < nk; ++k)
            (void)hipMemcpyAsync(c->rg.dbg.as<float>() + (size_t)rg_plane15(ref, ch, k) * n, rp.hbuf[s] + (size_t)(ch * nk + k) * n,
                                 n * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
}

// Positive-XYB planes of one frame at every scale, straight from its bytes: the band pyramid with
// XYB outputs (the recursive modes read nothing but XYB planes; no linear-light level is stored).
// `s16`: the frame is 16-bit (d_frame unused).
void rg_launch_convert(ssimu2_ctx* c, const Pyramid& p, const uint8_t* d_frame, const RgPlan& rp,
                       const Src16* s16 = nullptr) {
    const uint8_t* frames[1] = {d_frame};
    float* none[1] = {nullptr};
    PyrBandArgs a = pyramid_args(p, 1, frames, none);
    a.xyb0[0] = rp.xout[0];
    a.zero4 = rp.q;
    for (int l = 0; l < a.nlevels; ++l) a.out[0][l] = rp.xout[l + 1];
    for (int l = 0; l < p.nscales && l < 6; ++l) a.opitch[l] = rp.pitch[l];
    if (s16) {
        const PyrHbdArgs hb = hbd_args(1, &s16, nullptr);
        launch(s16->ch == 4 ? k_pyramid_bands_xyb16<4> : k_pyramid_bands_xyb16<3>, dim3(a.bands_x * a.bands_y),
               dim3(PYR_THREADS), 0, c->stream, a, hb);
        return;
    }
    launch(k_pyramid_bands_xyb, dim3(a.bands_x * a.bands_y), dim3(PYR_THREADS), 0, c->stream, a);
}

// Grid of the persistent vertical pass (k_rg_v, k_rg_vmap): one workgroup per CU, or per job where those are fewer.
dim3 rg_v_grid(const ssimu2_ctx* c, int vblocks) { return dim3(vblocks < c->num_cus ? vblocks : c->num_cus); }

// The horizontal pass: one workgroup per 20 rows and channel.
template <bool REF>
void rg_launch_h(ssimu2_ctx* c, bool fma, int hblocks, const RgPlan& rp) {
    if (hblocks <= 0) return;
    launch(fma ? k_rg_h<true, REF> : k_rg_h<false, REF>, dim3(hblocks), dim3(REF ? 128 : 192), 0, c->stream, rp);
}

// What depends on the reference alone: its XYB planes and mu1 = blur(x), s11 = blur(x * x) at
// every scale (the reference's linear pyramid is already enqueued).
void rg_enqueue_reference(ssimu2_ctx* c, const Pyramid& p, const uint8_t* d_ref, const Src16* s16 = nullptr) {
    RgPlan rp;
    int hblocks, vblocks;
    rg_build_plan(c, p, true, &rp, &hblocks, &vblocks);
    if (p.nscales == 0) return;  // a frame below 8 x 8 has no scale to score
    for (int s = 0; s < p.nscales; ++s) rp.emit[s] = rp.cache[s];
    const bool fma = c->blur_mode == SSIMU2_BLUR_RECURSIVE_FMA, dbg = rg_debugging(c, p);
    rg_launch_convert(c, p, d_ref, rp, s16);
    rg_launch_h<true>(c, fma, hblocks, rp);
    if (dbg) rg_debug_keep_h(c, p, rp, true);
    launch(fma ? k_rg_v_emit<true, 2> : k_rg_v_emit<false, 2>, dim3(vblocks), dim3(128), 0, c->stream, rp);
}

// The tail of every single score: the final reduction, which writes its 880 bytes straight into the context's
// page-locked mirror (no D2H copy command per score); ssimu2_wait collects it.
int finish_score(ssimu2_ctx* c, const FinalizeArgs& fa) {
    launch(k_finalize, dim3(1), dim3(1024), 0, c->stream, fa, c->h_result.as<double>());
    HIP_TRY(c, hipGetLastError());
    c->pending = true;
    return SSIMU2_OK;
}

// One pass against the reference planes in place: XYB of the distorted frame, the recursion over
// {y, y*y, x*y}, maps, final reduction (its linear pyramid is already enqueued).
int rg_enqueue_pass(ssimu2_ctx* c, const Pyramid& p, const uint8_t* d_dist, const Src16* s16 = nullptr) {
    RgPlan rp;
    int hblocks, vblocks;
    rg_build_plan(c, p, false, &rp, &hblocks, &vblocks);
    const bool fma = c->blur_mode == SSIMU2_BLUR_RECURSIVE_FMA, dbg = rg_debugging(c, p);
    FinalizeArgs fa = finalize_args(p);
    for (int s = 0; s < p.nscales; ++s) {
        fa.part[s] = rp.part[s];
        fa.nblocks[s] = rp.vgroups[s];  // one partial sum per column group
    }
    if (p.nscales > 0) {  // a frame below 8 x 8 has no scale to score
        rg_launch_convert(c, p, d_dist, rp, s16);
        rg_launch_h<false>(c, fma, hblocks, rp);
        launch(fma ? k_rg_v<true> : k_rg_v<false>, rg_v_grid(c, vblocks), dim3(512), c->rg_v_pad, c->stream, rp);
        if (dbg) {
            rg_debug_keep_h(c, p, rp, false);
            const int s = c->rg_dbg_scale;
            rp.emit[s] = c->rg.dbg.as<float>() + (size_t)15 * rg_pitch(p.w[s]) * p.h[s];  // [channel][{y, yy, xy}][n]
            launch(fma ? k_rg_v_emit<true, 3> : k_rg_v_emit<false, 3>, dim3(vblocks), dim3(192), 0, c->stream, rp);
        }
    }
    return finish_score(c, fa);
}

// Recursive modes, before anything of a score or reference is enqueued: the size limit and the planes.  `needs_ref`:
// the call scores against the cached reference, which growing the planes drops.
int rg_prepare(ssimu2_ctx* c, const Pyramid& p, uint32_t w, uint32_t h, bool needs_ref) {
    int rc = rg_check_size(c, w, h);
    if (rc) return rc;
    const bool had_ref = c->ref.have;
    if ((rc = rg_ensure(c, p))) return rc;
    if (needs_ref && had_ref && !c->ref.have)
        return c->fail(SSIMU2_ERR_NO_REFERENCE, "recursive blur mode: the cached reference was dropped");
    return SSIMU2_OK;
}

// What a pass against the cached reference is refused for once its arguments are in order, before anything of it is
// enqueued.  FIR: a 16-bit scale 0 (`hbd`) cannot be paired with an 8-bit reference frame in one marching kernel, so it
// needs the reference's cached planes.  Recursive modes: rg_prepare.
int pass_prepare(ssimu2_ctx* c, bool hbd) {
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (c->blur_mode != SSIMU2_BLUR_FIR) return rg_prepare(c, make_pyramid(w, h), w, h, true);
    if (hbd && !ref_cached(c))
        return c->fail(SSIMU2_ERR_OOM, "16-bit frames against a reference need its cached planes, which are missing");
    return SSIMU2_OK;
}

// Every launch of one score on the context stream, nothing refused any more: `dist` against `ref` (the same kind of
// frame), or with `ref` null against the cached reference (set from 8- or 16-bit samples; its planes do not depend on
// the depth).  16-bit frames take the same kernels after the front end: k_pyramid_bands16 (FIR, which also writes scale
// 0's linear planes for k_march_lin / k_march_refblur_lin) or k_pyramid_bands_xyb16 (recursive modes).
int launch_score(ssimu2_ctx* c, uint32_t w, uint32_t h, const Fed* ref, const Fed& dist) {
    const Pyramid p = make_pyramid(w, h);
    const bool hbd = !dist.u8;
    const uint8_t* const ref_u8 = ref ? ref->u8 : c->frame.ref_u8.as<uint8_t>();
    if (!hbd) note_lin0(c, 0, 0, w, h);  // an 8-bit score: the 16-bit scale-0 planes are older than it
    if (c->blur_mode != SSIMU2_BLUR_FIR) {  // straight to XYB planes; a cached reference's are in place
        if (ref) rg_enqueue_reference(c, p, ref_u8, hbd ? &ref->s16 : nullptr);
        return rg_enqueue_pass(c, p, dist.u8, hbd ? &dist.s16 : nullptr);
    }
    float* lin[2] = {c->frame.lin_ref.as<float>(), c->frame.lin_dist.as<float>()};
    const int skip = ref ? 0 : 1;  // against the cached reference: the distorted frame alone, its pyramid is ready
    MarchPlan mp;
    FinalizeArgs fa;
    if (hbd) {
        const Src16* src[2] = {ref ? &ref->s16 : nullptr, &dist.s16};
        float* lin0[2] = {c->hbd.lin0_ref.as<float>(), c->hbd.lin0_dist.as<float>()};
        launch_pyramid16(c, p, 2 - skip, src + skip, lin + skip, lin0 + skip);
        if (p.nscales >= 1) note_lin0(c, ref ? 1 : -1, 1, w, h);
        build_plans(c, p, march_seg_rows, score_sources(c, lin0[0], lin0[1], !ref), &mp, &fa);  // pass_prepare: cached
    } else {
        const uint8_t* frames[2] = {ref_u8, dist.u8};
        launch_pyramid(c, p, 2 - skip, frames + skip, lin + skip);
        build_plans(c, p, march_seg_rows, score_sources(c, ref_u8, dist.u8, !ref && c->cache.xyb.p), &mp, &fa);
    }
    launch_march(c, mp.ref_s11[0] != nullptr, hbd, mp);
    return finish_score(c, fa);
}

// Enqueue the whole score of two 8-bit frames on the device (the enqueue forms, the timing hooks): d_dist against
// d_ref, or with `against_ref` against the cached reference, whose 8-bit frame d_ref is.
int enqueue_score(ssimu2_ctx* c, const uint8_t* d_ref, const uint8_t* d_dist, uint32_t w, uint32_t h,
                  bool against_ref) {
    const int rc = c->blur_mode != SSIMU2_BLUR_FIR ? rg_prepare(c, make_pyramid(w, h), w, h, against_ref) : SSIMU2_OK;
    if (rc) return rc;
    const Fed ref{d_ref, {}}, dist{d_dist, {}};
    return launch_score(c, w, h, against_ref ? nullptr : &ref, dist);
}

// ---- sRGB -> linear tables (DESIGN.md sections 10 and 13) -----------------------------------------
// The table of the `n` codes 0..top (n = top + 1): the 8-bit table's expression at v = code / top, fp64, rounded once.
// 65535 = 255 * 257 and 65025 = 255 * 255, so entry 257 u of depth 16 and entry 255 u of the composite table are the
// 8-bit entry u bit for bit (v is the same double).  Built once per process and top code: the depths 8..16 and the
// composite table are ten.
const float* host_table(uint32_t n, uint32_t top) {
    static std::mutex mu;
    static struct {
        uint32_t top;
        const float* t;
    } built[16];
    static int nbuilt = 0;
    std::lock_guard<std::mutex> lock(mu);
    for (int k = 0; k < nbuilt; ++k)
        if (built[k].top == top) return built[k].t;
    float* t = nbuilt < 16 ? new (std::nothrow) float[n] : nullptr;
    if (!t) return nullptr;
    for (uint32_t i = 0; i < n; ++i) {
        const double v = (double)i / (double)top;
        t[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
    }
    built[nbuilt++] = {top, t};
    return t;
}

}  // namespace

// The tables as the exported functions hand them out.
int ssimu2h::copy_table(uint32_t n, uint32_t top, float* out) {
    if (!out) return SSIMU2_ERR_INVALID_ARG;
    const float* t = host_table(n, top);
    if (!t) return SSIMU2_ERR_OOM;
    memcpy(out, t, (size_t)n * sizeof(float));
    return SSIMU2_OK;
}

namespace {

size_t table_off(uint32_t d) { return ((size_t)1 << d) - 256; }

// The device copy of the table of `n` codes 0..top, uploaded on the context stream by the first call that needs it.
// A depth's table (n = 2^d) lies in `tab` at float offset 2^d - 256; any other is the composite table, alone in
// `alpha_tab`.
int device_table(ssimu2_ctx* c, uint32_t n, uint32_t top, const float** out) {
    const bool depth = (n & (n - 1)) == 0;
    DevBuf& buf = depth ? c->tab : c->alpha_tab;
    const size_t total = depth ? table_off(17) : n, off = depth ? n - 256 : 0;
    const uint32_t bit = depth ? n : 1u;  // of tab_ready
    const char* what = depth ? "hipMalloc(16-bit sRGB tables)" : "hipMalloc(composite table)";
    const int rc = grow(c, buf, total * sizeof(float), what);  // once per context
    if (rc) return rc;
    if (!(c->tab_ready & bit)) {
        const float* t = host_table(n, top);
        if (!t) return c->fail(SSIMU2_ERR_OOM, depth ? "16-bit sRGB table" : "composite table");
        HIP_TRY(c, hipMemcpyAsync(buf.as<float>() + off, t, (size_t)n * sizeof(float), hipMemcpyHostToDevice,
                                  c->stream));
        c->tab_ready |= bit;
    }
    *out = buf.as<float>() + off;
    return SSIMU2_OK;
}

// ---- a caller's frame onto the device ("One path for a frame"; Feed: ssimu2_host.h) ----
// Tight RGB frames of w pixels per row: 8-bit (u16 samples: ssimu2h::tight16 below).
Feed tight8(const void* px, uint32_t w, hipMemcpyKind kind = hipMemcpyHostToDevice) {
    return {{{px, w * 3u}}, 1u, kind, 3u, 1u, 0u, false, nullptr, -1};
}

// The slot's tight frame: ensure_capacity's 8-bit one, or the u16 one.
DevBuf& feed_frame(ssimu2_ctx* c, const Feed& f, bool ref) {
    return f.top ? (ref ? c->hbd.ref16 : c->hbd.dist16) : (ref ? c->frame.ref_u8 : c->frame.dist_u8);
}

// The last row needs only its pixels, not its padding (libavif allocates rowBytes * height, a cropped view of a larger
// buffer may not).  A plane with a size of its own (Plane::w, Plane::h) is that many rows of that many pixels.
size_t plane_bytes(const Feed& f, uint32_t p, uint32_t w, uint32_t h) {
    const Plane& pl = f.plane[p];
    return (size_t)pl.row_bytes * ((pl.h ? pl.h : h) - 1) + (size_t)(pl.w ? pl.w : w) * f.ch * f.sample;
}

}  // namespace

// A tight frame of u16 samples of depth `bit_depth` in host memory.
Feed ssimu2h::tight16(const void* px, uint32_t w, uint32_t bit_depth) {
    return {{{px, w * 6u}}, 1u, hipMemcpyHostToDevice, 3u, 2u, (1u << bit_depth) - 1u, false, nullptr, -1};
}

// Argument checks of the 16-bit calls (the ctx is not null).
int ssimu2h::check16(ssimu2_ctx* c, const void* px, uint32_t bit_depth) {
    if (!px) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer");
    if ((uintptr_t)px & 1u) return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit image pointer not 2-byte aligned");
    if (bit_depth < 8 || bit_depth > 16) return c->fail(SSIMU2_ERR_UNSUPPORTED, "bit_depth must be 8..16");
    return SSIMU2_OK;
}

// A frame of one plane in host memory, staged: rows `row_bytes` apart of `ch` samples of `sample` bytes per pixel.
Feed ssimu2h::staged1(const void* px, uint32_t row_bytes, uint32_t ch, uint32_t sample, uint32_t top,
                      void (*unpack)(ssimu2_ctx*, const Feed&, uint32_t, uint32_t, void*), int64_t bg) {
    return {{{px, row_bytes}}, 1u, hipMemcpyHostToDevice, ch, sample, top, true, unpack, bg};
}

// Where plane `p` lies in `stage`: the planes back to back, each start 16-byte aligned (plane 0 at 0).
size_t ssimu2h::plane_off(const Feed& f, uint32_t p, uint32_t w, uint32_t h) {
    size_t off = 0;
    for (uint32_t q = 0; q < p; ++q) off += (plane_bytes(f, q, w, h) + 15) & ~(size_t)15;
    return off;
}

namespace {
size_t feed_bytes(const Feed& f, uint32_t w, uint32_t h) {
    return plane_off(f, f.nplanes - 1, w, h) + plane_bytes(f, f.nplanes - 1, w, h);
}
}  // namespace

// Feeding a frame, first half: every buffer it needs beyond ensure_capacity's -- `stage` (16 bytes of slack behind the
// frame), and for u16 codes the slot's tight frame, in FIR mode its scale-0 linear planes, the table (fed->s16.tab).
// Enqueues nothing that reads the caller's memory, so a failure needs no wait.
int ssimu2h::feed_reserve(ssimu2_ctx* c, const Feed& f, bool ref, uint32_t w, uint32_t h, Fed* fed) {
    int rc;
    if (f.staged && (rc = grow(c, c->stage, feed_bytes(f, w, h) + 16, "hipMalloc(staging frame)"))) return rc;
    if (!f.top) return SSIMU2_OK;
    const size_t px = (size_t)w * h * 3;
    const bool in_stage = f.staged && !f.unpack;  // no tight frame
    if (!in_stage && (rc = grow(c, feed_frame(c, f, ref), px * sizeof(uint16_t), "hipMalloc(16-bit frames)")))
        return rc;
    note_lin0(c, ref ? 0 : -1, ref ? -1 : 0, w, h);  // the call may regrow or rewrite them: valid again once launched
    DevBuf& lin0 = ref ? c->hbd.lin0_ref : c->hbd.lin0_dist;
    if (c->blur_mode == SSIMU2_BLUR_FIR && (rc = grow(c, lin0, px * sizeof(float), "hipMalloc(16-bit scale-0 planes)")))
        return rc;
    return device_table(c, f.top + 1, f.top, &fed->s16.tab);
}

// Second half, after every feed_reserve of the call: the copy from the caller's memory and the unpacking, on the
// context stream; *fed is what the front end reads.
int ssimu2h::feed_enqueue(ssimu2_ctx* c, const Feed& f, bool ref, uint32_t w, uint32_t h, Fed* fed) {
    void* const frame = feed_frame(c, f, ref).p;
    uint8_t* const to = (uint8_t*)(f.staged ? c->stage.p : frame);  // a frame that is not staged has one plane
    for (uint32_t p = 0; p < f.nplanes; ++p)
        HIP_TRY(c, hipMemcpyAsync(to + plane_off(f, p, w, h), f.plane[p].px, plane_bytes(f, p, w, h), f.kind, c->stream));
    if (f.unpack) f.unpack(c, f, w, h, frame);
    fed->u8 = f.top ? nullptr : (const uint8_t*)frame;
    if (f.staged && !f.unpack) fed->s16 = {c->stage.p, f.plane[0].row_bytes, f.ch, fed->s16.tab, f.top};
    else fed->s16 = {frame, w * 6u, 3u, fed->s16.tab, f.top};
    return SSIMU2_OK;
}

// The one way out of a call from its first copy out of the caller's memory onwards: a failed call waits for the
// stream, so that the caller may free its frames after any return (a call that succeeds has waited for its result).
int ssimu2h::leave(ssimu2_ctx* c, int rc) {
    if (rc) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// The body of the front ends' diagnostics (ssimu2_composite_rgba8, ssimu2_convert_yuv), after their argument checks:
// the frame `f` of u16 codes goes into the distorted slot as in a score, and its w * h * 3 codes come back.
int ssimu2h::feed_codes(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, uint16_t* out_codes, const char* what) {
    HIP_TRY(c, hipSetDevice(c->device));
    Fed codes{};
    int rc = feed_reserve(c, f, false, w, h, &codes);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (!(rc = feed_enqueue(c, f, false, w, h, &codes)) &&  // the download is the diagnostics' alone
        ((e = hipGetLastError()) != hipSuccess ||
         (e = hipMemcpyAsync(out_codes, codes.s16.px, (size_t)w * h * 6, hipMemcpyDeviceToHost, c->stream)) ||
         (e = hipStreamSynchronize(c->stream)) != hipSuccess))
        rc = c->fail(SSIMU2_ERR_HIP, what, e);
    return leave(c, rc);
}

namespace {

// ---- error map --------------------------------------------------------------
// Coefficients of the map's terms from the averages of the score that just finished (h_result): the weight of
// every average by the score's contiguous walk (k_finalize, or_score_from_averages), w for an L1 term and
// w / a^3 for an L4 term (0 when a == 0), so that the mean of each term's density is w * a.
void map_coefficients(const ssimu2_ctx* c, int nscales, MapCoef* mc) {
    memset(mc, 0, sizeof *mc);
    int j = 0;
    for (int ch = 0; ch < 3; ++ch)
        for (int sc = 0; sc < nscales; ++sc)
            for (int n = 0; n < 2; ++n)
                for (int k = 0; k < 3; ++k, ++j) {
                    const int stat = k == 0 ? ch * 2 + n : 6 + ch * 4 + n + (k == 2 ? 2 : 0);
                    const double a = c->h_result.as<double>()[sc * kStats + stat], wt = kWeightsHost[j];
                    double v = n == 0 ? wt : (a > 0.0 ? wt / (a * a * a) : 0.0);
                    if (v > 3.0e38) v = 3.0e38;  // a nonzero L4 average below ~1e-13 (denormal terms): stay finite
                    mc->c[sc][stat] = (float)v;
                }
}

// The map buffers for this frame size: allocated on first use, replaced when the size DIFFERS (not only when it is
// larger: a map of a small frame does not sit on a large frame's planes); a failure leaves both released.
int map_ensure(ssimu2_ctx* c, const Pyramid& p, uint32_t w, uint32_t h) {
    const size_t need_dens = (xyb_off(p, p.nscales) + 4) * sizeof(float), need_map = (size_t)w * h * sizeof(float);
    if (c->map.out.p && need_dens == c->map.dens.cap && need_map == c->map.out.cap) return SSIMU2_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    release(c->map);
    const char* what = "hipMalloc(error map: 20 bytes per pixel)";
    int rc;
    if ((rc = grow(c, c->map.dens, need_dens, what)) || (rc = grow(c, c->map.out, need_map, what))) release(c->map);
    return rc;
}

// The map pass after a finished score (its planes still in place): densities of every scale from the same per-pixel
// terms, composed into the w x h map, downloaded into `out_map`.  `hbd` says what the score read at scale 0, which the
// FIR pass reads again: two 8-bit frames (the context's ref_u8 / dist_u8), or the 16-bit path's linear planes
// hbd.lin0_ref / hbd.lin0_dist; the scales below come from the lin_ref / lin_dist pyramids either way, and the
// recursive modes read the planes of rg.planes, whatever made them.  Reads the score's buffers and writes only the
// map's own: the averages, partial sums and a cached reference are left as the score left them.
int map_pass(ssimu2_ctx* c, bool hbd, uint32_t w, uint32_t h, float* out_map) {
    const Pyramid p = make_pyramid(w, h);
    int rc = map_ensure(c, p, w, h);
    if (rc) return rc;
    const size_t npix = (size_t)w * h;
    float* const dens = c->map.dens.as<float>();
    if (p.nscales == 0) {  // a frame below 8 x 8 has no scale: the map is zero, as the score is 100
        HIP_TRY(c, hipMemsetAsync(c->map.out.p, 0, npix * sizeof(float), c->stream));
    } else {
        MapCoef mc;
        map_coefficients(c, p.nscales, &mc);
        if (c->blur_mode == SSIMU2_BLUR_FIR) {
            MarchPlan mp;
            FinalizeArgs fa;
            PlanSources src = hbd ? score_sources(c, c->hbd.lin0_ref.p, c->hbd.lin0_dist.p, false)
                                  : score_sources(c, c->frame.ref_u8.p, c->frame.dist_u8.p, false);
            src.ref_s11 = dens;  // the output planes
            const int blocks = build_plans(c, p, march_seg_rows, src, &mp, &fa, MARCH_OUT_PLANES);
            launch(hbd ? k_march_map_lin : k_march_map, dim3(blocks), dim3(MARCH_THREADS), 0, c->stream, mp, mc);
        } else {
            RgPlan rp;
            int hblocks, vblocks;
            rg_build_plan(c, p, false, &rp, &hblocks, &vblocks);
            RgMapArgs ma;
            memset(&ma, 0, sizeof ma);
            ma.coef = mc;
            for (int s = 0; s < p.nscales; ++s) ma.dens[s] = dens + xyb_off(p, s);
            HIP_TRY(c, hipMemsetAsync(c->d_rg_q, 0, 4 * sizeof(unsigned), c->stream));  // the job cursor
            launch(c->blur_mode == SSIMU2_BLUR_RECURSIVE_FMA ? k_rg_vmap<true> : k_rg_vmap<false>, rg_v_grid(c, vblocks),
                   dim3(512), c->rg_v_pad, c->stream, rp, ma);
        }
        MapComposeArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.nscales = p.nscales;
        for (int s = 0; s < p.nscales; ++s) {
            ca.dens[s] = dens + xyb_off(p, s);
            ca.w[s] = p.w[s];
            ca.h[s] = p.h[s];
        }
        ca.out = c->map.out.as<float>();
        launch(k_map_compose, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream, ca);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out_map, c->map.out.p, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SSIMU2_OK;
}

}  // namespace

int ssimu2h::check_args(ssimu2_ctx* c, const void* a, const void* b, uint32_t w, uint32_t h) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!a || !b) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer");
    if (w == 0 || h == 0) return c->fail(SSIMU2_ERR_INVALID_ARG, "zero image dimension");
    if ((uint64_t)w * h > (1ull << 31) / 3)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "image larger than 2^31/3 pixels");
    return SSIMU2_OK;
}

namespace {

// ---- batch scoring (include/ssimu2_hip.h "Batch scoring") -------------------
constexpr size_t kResultDoubles = kNumScales * kStats + 2;  // one item's block of the result mirror

// The opening of the four batch entry points, used as `if (rc || n == 0) return rc;`: a null context, an empty batch
// (SSIMU2_OK, nothing else is looked at), then what every batch call refuses.
// `any_mode`: the calls of include/ssimu2_hip_rbatch.h, which batch in the recursive modes too (rbatch_open).
int batch_open(ssimu2_ctx* c, uint32_t n, bool against_reference, bool any_mode = false) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (n == 0) return SSIMU2_OK;
    if (!any_mode && c->blur_mode != SSIMU2_BLUR_FIR)
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "batch scoring runs in SSIMU2_BLUR_FIR only: switch the context with "
                                               "ssimu2_ctx_set_blur, or score the pairs one by one");
    if (against_reference && !c->ref.have) return c->fail(SSIMU2_ERR_NO_REFERENCE, "no reference set");
    if (n > SSIMU2_MAX_BATCH) return c->fail(SSIMU2_ERR_INVALID_ARG, "batch larger than SSIMU2_MAX_BATCH items");
    return SSIMU2_OK;
}

// Score n device-resident items of w x h: d_dists + i * dist_stride0 against d_refs + i * ref_stride0, or (d_refs
// null) against the context's cached reference.  ONE k_pyramid_bands_batch, ONE k_march_batch / k_march_refblur_batch,
// ONE k_finalize_batch, one synchronise; whatever was enqueued on the stream before (uploads) comes first.
int batch_run(ssimu2_ctx* c, const uint8_t* d_refs, const uint8_t* d_dists, size_t stride0, uint32_t n, uint32_t w,
              uint32_t h, double* out_scores) {
    const bool against_ref = d_refs == nullptr;
    const Pyramid p = make_pyramid(w, h);
    MarchBatchPlan bp;
    FinalizeArgs fa;
    memset(&bp, 0, sizeof bp);
    MarchPlan& mp = bp.item;
    const long long blocks = build_plans(c, p, batch_seg_rows, {}, &mp, &fa);  // the sizes
    const size_t part_stride = (size_t)blocks * kStats;  // doubles between items' partial sums
    const int nframes = against_ref ? 1 : 2;
    const long long bands = (long long)((p.w[0] + PYR_BAND_W - 1) / PYR_BAND_W) * ((p.h[0] + PYR_BAND_H - 1) / PYR_BAND_H);
    if (blocks * n > 0x7fffffffLL || bands * nframes * n > 0x7fffffffLL)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "batch too large for one launch: fewer items per call");
    const bool cached = against_ref && ref_cached(c);
    if (against_ref && !cached && c->ref.hbd)  // as ssimu2_score_against_reference_rgb16: no 8-bit frame of that reference
        return c->fail(SSIMU2_ERR_OOM, "a batch against a 16-bit reference needs its cached planes, which are missing");
    const size_t lin_stride = (p.lin_total + 3) & ~(size_t)3;  // floats between items' pyramids
    auto& b = c->batch;
    const size_t lin_bytes = (size_t)n * lin_stride * sizeof(float) + 16, res_bytes = (size_t)n * kResultDoubles * sizeof(double);
    int rc;
    if ((rc = grow(c, b.lin_dist, lin_bytes, "hipMalloc(batch pyramids)")) ||
        (!against_ref && (rc = grow(c, b.lin_ref, lin_bytes, "hipMalloc(batch pyramids)"))) ||
        (rc = grow(c, b.part, ((size_t)n * part_stride + 8) * sizeof(double), "hipMalloc(batch partial sums)")))
        return rc;
    // the page-locked result block (k_finalize_batch writes it over the bus itself, as k_finalize does); regrowing it
    // takes the last batch's averages with it
    if (!fits(b.result, res_bytes)) c->batch_n = 0;
    if ((rc = grow(c, b.result, res_bytes, "hipHostMalloc(batch results)"))) return rc;
    PlanSources src = score_sources(c, against_ref ? c->frame.ref_u8.p : d_refs, d_dists, cached);
    if (!against_ref) src.lin_ref = b.lin_ref.as<float>();
    src.lin_dist = b.lin_dist.as<float>();
    src.part = b.part.as<double>();
    build_plans(c, p, batch_seg_rows, src, &mp, &fa);  // item 0; the others lie the strides below behind it
    for (int s = 0; s < p.nscales; ++s) bp.blk_end[s] = (int)(mp.blk_end[s] * (long long)n);
    bp.n_items = (int)n;
    bp.ref_stride0 = against_ref ? 0 : stride0;  // one reference for all items
    bp.dist_stride0 = stride0;
    bp.ref_stride = against_ref ? 0 : lin_stride * sizeof(float);
    bp.dist_stride = lin_stride * sizeof(float);
    bp.part_stride = part_stride;
    if (p.nscales > 1) {
        const uint8_t* frames[2] = {against_ref ? d_dists : d_refs, d_dists};
        float* lin[2] = {against_ref ? b.lin_dist.as<float>() : b.lin_ref.as<float>(), b.lin_dist.as<float>()};
        PyrBatchArgs pb;
        pb.a = pyramid_args(p, nframes, frames, lin);
        pb.in_stride = stride0;
        pb.out_stride = lin_stride;
        launch(k_pyramid_bands_batch, dim3((unsigned)(bands * nframes * n)), dim3(PYR_THREADS), 0, c->stream, pb);
    }
    launch_march(c, cached, false, mp, &bp);
    launch(k_finalize_batch, dim3(n), dim3(1024), 0, c->stream, fa, part_stride, b.result.as<double>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->batch_n = n;
    for (uint32_t i = 0; i < n; ++i) out_scores[i] = b.result.as<double>()[(size_t)i * kResultDoubles + 108];
    return SSIMU2_OK;
}

// Upload n host frames into a staging buffer of the context, `stride` bytes apart, on the context stream.
int batch_stage(ssimu2_ctx* c, DevBuf& buf, const uint8_t* const* frames, uint32_t n, size_t bytes, size_t stride) {
    int rc = grow(c, buf, (size_t)n * stride + 16, "hipMalloc(batch frames)");
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i)
        HIP_TRY(c, hipMemcpyAsync(buf.as<uint8_t>() + (size_t)i * stride, frames[i], bytes, hipMemcpyHostToDevice, c->stream));
    return SSIMU2_OK;
}

// ---- batches in the recursive modes (include/ssimu2_hip_rbatch.h) ------------
// Floats behind the batch's last plane that no kernel writes and k_rg_h_batch may read.  rg_h_fetch is unconditional:
// while a wave works on tile T it fetches tile T + AHEAD, and the last tile it works on is ntiles - 1 with ntiles =
// ceil((w + 4) / 64).  64 * ntiles is a multiple of 64 below w + 68 <= pitch + 68, so at most pitch + 64; the farthest
// column fetched is 64 * (ntiles - 1 + AHEAD) + 63 <= pitch + 64 * AHEAD + 63.  In the plane's last row, h - 1, that
// is 64 * (AHEAD + 1) floats behind the plane's end at the most, and AHEAD is RG_H_AHEAD_REF = 2 in the reference's
// pass, the larger of the two.  The last plane a wave reads of the last item (xb's third; xa's third in the
// reference's pass) has that item's later planes and the dump row behind it in this layout; the slack covers it
// wherever it lies.
constexpr size_t kRgBatchTail = (size_t)RG_TW * (RG_H_AHEAD_REF + 1);

// Where the frames of a recursive batch lie on the device: item i's reference at refs + i * stride0 (null: every item
// against the cached reference), its distorted frame at dists + i * stride0.  s16 null: tight 8-bit RGB; else tight
// 16-bit frames read as *s16 describes (pitch, channels, table, top code; its px is not looked at).
struct BatchFrames {
    const void *refs, *dists;
    size_t stride0;
    const Src16* s16;
};

long long rg_batch_bands(uint32_t w, uint32_t h) {
    return (long long)((w + PYR_BAND_W - 1) / PYR_BAND_W) * ((h + PYR_BAND_H - 1) / PYR_BAND_H);
}

// What a recursive batch is refused for once its sizes are known, before anything is allocated or enqueued: a grid or a
// job count of one of its launches beyond 2^31 - 1.  `one`: an item's counts; `bands`: an item's conversion workgroups.
int rg_batch_check_launch(ssimu2_ctx* c, const RgCounts& one, long long bands, uint32_t n) {
    if ((long long)one.hblocks * n > 0x7fffffffLL || (long long)one.vblocks * n > 0x7fffffffLL || bands * n > 0x7fffffffLL)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "batch too large for one launch: fewer items per call");
    return SSIMU2_OK;
}

// n items of w x h in SSIMU2_BLUR_RECURSIVE / _FMA: ONE k_pyramid_bands_xyb_batch, (pair form: ONE k_rg_h_batch<REF>
// and ONE k_rg_v_emit_batch for the references,) ONE k_rg_h_batch, ONE k_rg_v_batch, ONE k_finalize_batch, one
// synchronise.  Item i's planes are one block of the batch's own scratch -- pair form [xa 3][xb 3][cache 6][hbuf 9]
// planes of every scale, against form [xb 3][hbuf 9] with xa and cache the context's cached reference (stride 0) --
// each laid out inside as rg_build_plan lays the context's, so an item's jobs see the geometry of its single score.
// Where the items' frames come from (`fr`): 8-bit bytes or 16-bit frames (ssimu2_hbatch_*), for
// which the one conversion launch is k_pyramid_bands_xyb16_batch.  Nothing behind the conversion knows which it was.
int rbatch_recursive(ssimu2_ctx* c, const BatchFrames& fr, uint32_t n, uint32_t w, uint32_t h, double* out_scores) {
    const bool against_ref = fr.refs == nullptr;
    const size_t stride0 = fr.stride0;
    const Pyramid p = make_pyramid(w, h);
    const size_t ntot = rg_plane_off(p, p.nscales);
    const size_t item_planes = (against_ref ? 12 : 21) * ntot;  // floats between items
    RgBatchPlan bp;
    memset(&bp, 0, sizeof bp);
    RgPlan& rp = bp.item;
    const RgCounts one = rg_plan_geometry(p, &rp);
    const long long hb = one.hblocks, vb = one.vblocks;
    const size_t part_stride = one.part;
    const int nframes = against_ref ? 1 : 2;
    const long long bands = rg_batch_bands(w, h);
    int rc;
    if ((rc = rg_batch_check_launch(c, one, bands * nframes, n))) return rc;
    auto& b = c->batch;
    const size_t dump_floats = p.nscales > 0 ? (size_t)rg_pitch(p.w[0]) + 16 : 16;
    const size_t res_bytes = (size_t)n * kResultDoubles * sizeof(double);
    if ((rc = grow(c, b.rg_planes, ((size_t)n * item_planes + dump_floats + kRgBatchTail) * sizeof(float),
                   "hipMalloc(recursive batch planes: 84 bytes per pixel, scale and item; 48 against a reference)")) ||
        (rc = grow(c, b.rg_part, 16 + ((size_t)n * part_stride + 8) * sizeof(double), "hipMalloc(recursive batch partial sums)")))
        return rc;
    if (!fits(b.result, res_bytes)) c->batch_n = 0;  // as batch_run: regrowing takes the last batch's averages with it
    if ((rc = grow(c, b.result, res_bytes, "hipHostMalloc(batch results)"))) return rc;

    float* const base = b.rg_planes.as<float>();
    float* const own_xa = base;                                     // pair form only
    float* const xb = against_ref ? base : base + 3 * ntot;
    float* const own_cache = xb + 3 * ntot;                         // pair form only
    float* const hbuf = against_ref ? xb + 3 * ntot : own_cache + 6 * ntot;
    // the cached reference: where rg_build_plan puts the context's xa and cache planes (read only here)
    float* const ref_xa = against_ref ? c->rg.planes.as<float>() : own_xa;
    float* const ref_cache = against_ref ? c->rg.planes.as<float>() + 6 * ntot : own_cache;
    rg_plan_buffers(p, &rp, ref_xa, xb, ref_cache, hbuf, (double*)(b.rg_part.as<char>() + 16));
    FinalizeArgs fa = finalize_args(p);
    for (int s = 0; s < p.nscales; ++s) {
        bp.hblk_end[s] = (int)(rp.hblk_end[s] * (long long)n);
        bp.vblk_end[s] = (int)(rp.vblk_end[s] * (long long)n);
        rp.emit[s] = against_ref ? nullptr : rp.cache[s];  // the pair form's k_rg_v_emit_batch writes the items' cache planes
        fa.part[s] = rp.part[s];
        fa.nblocks[s] = rp.vgroups[s];  // one partial sum per column group, as rg_enqueue_pass
    }
    rp.dump = base + (size_t)n * item_planes;
    rp.q = b.rg_part.as<unsigned>();
    bp.n_items = (int)n;
    bp.vjobs = (int)(vb * n);
    bp.items_fastest = against_ref;
    bp.xa_stride = against_ref ? 0 : item_planes;
    bp.cache_stride = against_ref ? 0 : item_planes;
    bp.xb_stride = bp.hbuf_stride = item_planes;
    bp.part_stride = part_stride;
    if (p.nscales > 0) {  // a frame below 8 x 8 has no scale to score
        const bool fma = c->blur_mode == SSIMU2_BLUR_RECURSIVE_FMA;
        const uint8_t* const d_dists = (const uint8_t*)fr.dists;
        const uint8_t* frames[2] = {against_ref ? d_dists : (const uint8_t*)fr.refs, d_dists};
        float* none[2] = {nullptr, nullptr};
        PyrBatchArgs pb;
        pb.a = pyramid_args(p, nframes, frames, none);
        for (int f = 0; f < nframes; ++f) {
            float* x = f == 0 && !against_ref ? own_xa : xb;
            for (int l = 0; l < p.nscales; ++l) (l == 0 ? pb.a.xyb0[f] : pb.a.out[f][l - 1]) = x + 3 * rg_plane_off(p, l);
        }
        for (int l = 0; l < p.nscales; ++l) pb.a.opitch[l] = rp.pitch[l];
        pb.a.zero4 = rp.q;
        pb.in_stride = stride0;
        pb.out_stride = item_planes;
        if (fr.s16) {  // both sides are read as *fr.s16 says: its pitch, table and top code, from their own first byte
            Src16 ref16 = *fr.s16, dist16 = *fr.s16;
            ref16.px = fr.refs, dist16.px = fr.dists;
            const Src16* src[2] = {against_ref ? &dist16 : &ref16, &dist16};
            const PyrHbdArgs hbd = hbd_args(nframes, src, nullptr);
            launch(k_pyramid_bands_xyb16_batch<3>, dim3((unsigned)(bands * nframes * n)), dim3(PYR_THREADS), 0, c->stream, pb, hbd);
        } else {
            launch(k_pyramid_bands_xyb_batch, dim3((unsigned)(bands * nframes * n)), dim3(PYR_THREADS), 0, c->stream, pb);
        }
        if (!against_ref) {
            launch(fma ? k_rg_h_batch<true, true> : k_rg_h_batch<false, true>, dim3((unsigned)(hb * n)), dim3(128), 0, c->stream, bp);
            launch(fma ? k_rg_v_emit_batch<true, 2> : k_rg_v_emit_batch<false, 2>, dim3((unsigned)(vb * n)), dim3(128), 0, c->stream, bp);
        }
        launch(fma ? k_rg_h_batch<true, false> : k_rg_h_batch<false, false>, dim3((unsigned)(hb * n)), dim3(192), 0, c->stream, bp);
        const int cus = c->dev.compute_units > 0 ? (int)c->dev.compute_units : 256;  // one workgroup per CU, as k_rg_v
        launch(fma ? k_rg_v_batch<true> : k_rg_v_batch<false>, dim3((unsigned)(vb * n < cus ? vb * n : cus)), dim3(512),
               c->rg_v_pad, c->stream, bp);
    }
    launch(k_finalize_batch, dim3(n), dim3(1024), 0, c->stream, fa, part_stride, b.result.as<double>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->batch_n = n;
    for (uint32_t i = 0; i < n; ++i) out_scores[i] = b.result.as<double>()[(size_t)i * kResultDoubles + 108];
    return SSIMU2_OK;
}

}  // namespace

int ssimu2h::rbatch_open(ssimu2_ctx* c, uint32_t n, bool against_reference) { return batch_open(c, n, against_reference, true); }

int ssimu2h::rbatch_check_size(ssimu2_ctx* c, uint32_t w, uint32_t h) {
    return c->blur_mode != SSIMU2_BLUR_FIR ? rg_check_size(c, w, h) : SSIMU2_OK;
}

int ssimu2h::rbatch_stage(ssimu2_ctx* c, bool ref, const uint8_t* const* frames, uint32_t n, size_t bytes, size_t stride,
                          const uint8_t** d_frames) {
    DevBuf& buf = ref ? c->batch.u8_ref : c->batch.u8_dist;
    const int rc = batch_stage(c, buf, frames, n, bytes, stride);
    *d_frames = buf.as<uint8_t>();
    return rc;
}

int ssimu2h::rbatch_run(ssimu2_ctx* c, const uint8_t* d_refs, const uint8_t* d_dists, size_t stride0, uint32_t n, uint32_t w,
                        uint32_t h, double* out_scores) {
    if (c->blur_mode == SSIMU2_BLUR_FIR) return batch_run(c, d_refs, d_dists, stride0, n, w, h, out_scores);
    return rbatch_recursive(c, {d_refs, d_dists, stride0, nullptr}, n, w, h, out_scores);
}

// ---- 16-bit and YUV batches (include/ssimu2_hip_hbatch.h) -------------------
int ssimu2h::hbatch_buffer(ssimu2_ctx* c, int which, size_t bytes, uint8_t** d_buf) {
    DevBuf& buf = which == 0 ? c->batch.h16_ref : which == 1 ? c->batch.h16_dist : c->batch.yuv_planes;
    const int rc = grow(c, buf, bytes + 16, "hipMalloc(16-bit batch frames)");
    *d_buf = buf.as<uint8_t>();
    return rc;
}

int ssimu2h::hbatch_table(ssimu2_ctx* c, uint32_t depth, const float** tab) {
    return device_table(c, 1u << depth, (1u << depth) - 1u, tab);
}

int ssimu2h::hbatch_run(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t stride0, uint32_t n, uint32_t w,
                        uint32_t h, const float* tab, uint32_t depth, double* out_scores) {
    const Src16 tight{nullptr, w * 6u, 3u, tab, (1u << depth) - 1u};
    return rbatch_recursive(c, {d_refs, d_dists, stride0, &tight}, n, w, h, out_scores);
}

// ---- RGBA and YUV-with-alpha batches (include/ssimu2_hip_abatch.h) ----------
int ssimu2h::abatch_run(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t stride0, uint32_t n, uint32_t w,
                        uint32_t h, double* out_scores) {
    constexpr uint32_t top = 65025;  // 255 * 255, the largest composite code
    const float* tab;
    const int rc = device_table(c, top + 1, top, &tab);
    if (rc) return rc;
    const Src16 tight{nullptr, w * 6u, 3u, tab, top};
    return rbatch_recursive(c, {d_refs, d_dists, stride0, &tight}, n, w, h, out_scores);
}

int ssimu2h::hbatch_check_launch(ssimu2_ctx* c, uint32_t n, uint32_t w, uint32_t h, bool against_reference) {
    RgPlan rp;
    const RgCounts one = rg_plan_geometry(make_pyramid(w, h), &rp);
    return rg_batch_check_launch(c, one, rg_batch_bands(w, h) * (against_reference ? 1 : 2), n);
}

extern "C" {

const char* ssimu2_version(void) { return "oavif_amd ssimu2 gfx950 v8 (pair ring, b64 taps, dword pixel loads; recursive blur: cached reference, 3 lanes per line, persistent vertical pass; placed streams; tagged option structs; device check at context creation; pinned host buffers)"; }

int ssimu2_ctx_set_blur(ssimu2_ctx* c, int mode) {
    REMOTE(c, set_blur(c->remote, mode));
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (mode != SSIMU2_BLUR_FIR && mode != SSIMU2_BLUR_RECURSIVE && mode != SSIMU2_BLUR_RECURSIVE_FMA)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "unknown blur mode");
    if (c->pending) return c->fail(SSIMU2_ERR_INVALID_ARG, "ssimu2_ctx_set_blur: a score is still enqueued");
    if (mode == SSIMU2_BLUR_FIR && c->rg.planes.p) {  // the recursive modes' planes are of no use to the default mode
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        release_recursive(c);
    }
    c->blur_mode = mode;
    c->ref.drop();
    return SSIMU2_OK;
}

const char* ssimu2_last_error(const ssimu2_ctx* ctx) {
    REMOTE(ctx, last_error(ctx->remote));
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

static int ctx_create_impl(int device, void* hip_stream, ssimu2_ctx** out_ctx);

}  // extern "C"

// ---- stream placement ---------------------------------------------------------------------------
// HIP maps streams onto a few hardware queues, and two streams that share one do not overlap at
// all: of six contexts created back to back on an MI355X the pairs (0,5), (1,4), (2,3) score at the
// one-stream rate, every other pair 13 % faster (scripts/gpu_stream_pairs.py).  A caller that
// scores independent frames on two contexts (a batch, speculative probes) cannot see this, so the
// library places the streams: once per process and device it creates a few candidate streams,
// runs short dependent spin kernels on pairs of them and keeps a set whose members all ran
// CONCURRENTLY with each other.  Contexts created without a caller stream borrow the first free
// member of that set (exclusively; ssimu2_ctx_destroy returns it), and only contexts beyond the
// set get a stream of their own on whatever queue HIP picks.
namespace {

__global__ void k_spin(long long ticks) {  // one wave; wall_clock64 runs at 100 MHz
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

constexpr int kPoolCandidates = 6, kPoolMax = 4;
struct StreamPool {
    bool built = false;
    int n = 0;
    hipStream_t stream[kPoolMax] = {nullptr, nullptr, nullptr, nullptr};
    bool in_use[kPoolMax] = {false, false, false, false};
};
std::mutex g_pool_mu;
StreamPool g_pool[64];

// Do streams a and b overlap their work?  Two dependent 100 us spin kernels on each, enqueued
// alternately.  Kernels of ONE stream are ordered by barrier packets, and a barrier packet waits
// for everything enqueued before it on its hardware queue -- the other stream's kernels too, if
// the two streams share the queue: >= 300 us then, 200 us on distinct queues.  (One kernel per
// stream proves nothing: without a barrier between them two packets of one queue run side by side.)
bool streams_overlap(hipStream_t a, hipStream_t b) {
    // Timed on the DEVICE (events on the two streams), best of four: a host clock around launch and
    // synchronize adds the launch path and the wake-up of the waiting thread to a 200-vs-300 us
    // decision, and one misread on a loaded host shrank the set to a single stream.
    const long long ticks = 10000;  // 100 us
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&ea) != hipSuccess || hipEventCreate(&eb) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        if (ea) (void)hipEventDestroy(ea);
        (void)hipGetLastError();
        return false;
    }
    double best = 1e9;
    for (int rep = 0; rep < 4; ++rep) {
        (void)hipStreamSynchronize(a);
        (void)hipStreamSynchronize(b);
        (void)hipEventRecord(e0, a);
        for (int k = 0; k < 2; ++k) {
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, ticks);
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, b, ticks);
        }
        (void)hipEventRecord(ea, a);
        (void)hipEventRecord(eb, b);
        (void)hipStreamSynchronize(a);
        (void)hipStreamSynchronize(b);
        float ma = 0.f, mb = 0.f;
        if (hipEventElapsedTime(&ma, e0, ea) != hipSuccess || hipEventElapsedTime(&mb, e0, eb) != hipSuccess) continue;
        const double us = 1e3 * (ma > mb ? ma : mb);
        if (us < best) best = us;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    (void)hipGetLastError();
    return best < 260.0;
}

// caller holds g_pool_mu and has set the device
void build_pool(StreamPool& pool) {
    pool.built = true;
    hipStream_t cand[kPoolCandidates];
    int nc = 0;
    for (; nc < kPoolCandidates; ++nc)
        if (hipStreamCreateWithFlags(&cand[nc], hipStreamNonBlocking) != hipSuccess) break;
    if (nc > 0) {  // code object load and clocks, untimed
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, cand[0], 2000LL);
        (void)hipStreamSynchronize(cand[0]);
    }
    bool keep[kPoolCandidates] = {false};
    for (int i = 0; i < nc && pool.n < kPoolMax; ++i) {
        bool ok = true;
        for (int j = 0; j < pool.n && ok; ++j) ok = streams_overlap(pool.stream[j], cand[i]);
        if (ok) {
            pool.stream[pool.n++] = cand[i];
            keep[i] = true;
        }
    }
    for (int i = 0; i < nc; ++i)
        if (!keep[i]) (void)hipStreamDestroy(cand[i]);
    (void)hipGetLastError();
}

hipStream_t pool_acquire(int device) {
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_pool_mu);
    StreamPool& pool = g_pool[device];
    if (!pool.built) build_pool(pool);
    for (int i = 0; i < pool.n; ++i)
        if (!pool.in_use[i]) {
            pool.in_use[i] = true;
            return pool.stream[i];
        }
    return nullptr;
}

// streams of the placed set of `device` (0 before the first context without a caller stream exists)
int pool_size(int device) {
    if (device < 0 || device >= 64) return 0;
    std::lock_guard<std::mutex> lock(g_pool_mu);
    return g_pool[device].n;
}

void pool_release(int device, hipStream_t s) {
    if (device < 0 || device >= 64) return;
    std::lock_guard<std::mutex> lock(g_pool_mu);
    StreamPool& pool = g_pool[device];
    for (int i = 0; i < pool.n; ++i)
        if (pool.stream[i] == s) pool.in_use[i] = false;
}

}  // namespace

extern "C" {

// ssimu2_prefetch: the once-per-process cost of the scorer (HIP runtime initialisation, loading
// the code object, the constant table: 140-340 ms on the MI355X box, scripts/gpu_coldstart.py) on
// a background thread, so that a one-image run hides it behind its image load and first encode.
static std::mutex g_prefetch_mu;
static std::shared_future<void> g_prefetch[64];

int ssimu2_prefetch(int device) {
    if (ssimu2r::enabled()) return device < 0 || device >= 64 ? SSIMU2_ERR_INVALID_ARG : SSIMU2_OK;  // HIP is not started
    if (device < 0 || device >= 64) return SSIMU2_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(g_prefetch_mu);
    if (g_prefetch[device].valid()) return SSIMU2_OK;
    try {
        g_prefetch[device] = std::async(std::launch::async, [device] {
            ssimu2_ctx* tmp = nullptr;  // a throw-away context does all of the above
            if (ctx_create_impl(device, nullptr, &tmp) == SSIMU2_OK) ssimu2_ctx_destroy(tmp);
        }).share();
    } catch (...) {
        return SSIMU2_ERR_OOM;
    }
    return SSIMU2_OK;
}

int ssimu2_prefetch_join(int device) {
    if (ssimu2r::enabled()) return device < 0 || device >= 64 ? SSIMU2_ERR_INVALID_ARG : SSIMU2_OK;
    if (device < 0 || device >= 64) return SSIMU2_ERR_INVALID_ARG;
    std::shared_future<void> f;
    {
        std::lock_guard<std::mutex> lock(g_prefetch_mu);
        f = g_prefetch[device];
    }
    if (f.valid()) f.wait();
    return SSIMU2_OK;
}

// OAVIF_SCORER_SOCKET is set: the context is a connection to the scoring service, and this process makes no HIP call
// for it.  No fallback to a local GPU when the service cannot be reached.
static int remote_create(int device, void* hip_stream, ssimu2_ctx** out_ctx) {
    if (!out_ctx) return SSIMU2_ERR_INVALID_ARG;
    *out_ctx = nullptr;
    ssimu2_ctx* c = new (std::nothrow) ssimu2_ctx();
    if (!c) return SSIMU2_ERR_OOM;
    c->device = device;
    const int rc = ssimu2r::create(device, hip_stream, ssimu2_version(), &c->remote, &c->dev, &g_create_error);
    if (rc != SSIMU2_OK) {
        delete c;
        return rc;
    }
    *out_ctx = c;
    return SSIMU2_OK;
}

int ssimu2_ctx_create(int device, void* hip_stream, ssimu2_ctx** out_ctx) {
    if (ssimu2r::enabled()) return remote_create(device, hip_stream, out_ctx);
    if (device >= 0 && device < 64) {
        std::shared_future<void> f;
        {
            std::lock_guard<std::mutex> lock(g_prefetch_mu);
            f = g_prefetch[device];
        }
        if (f.valid()) f.wait();  // a prefetch in flight finishes first
    }
    return ctx_create_impl(device, hip_stream, out_ctx);
}

// What the runtime and sysfs say of HIP device `device`; `why` (optional) receives the reason when the device is not
// one this library can run on.  No context, no allocation; hipGetDeviceProperties initialises the runtime.
static int query_device_impl(int device, ssimu2_device_info* d, std::string* why) {
    static std::mutex mu;                      // contexts are created from worker threads: one record per device,
    static ssimu2_device_info accepted[64];    // read from the runtime and sysfs once
    static bool have[64] = {false};
    std::lock_guard<std::mutex> lock(mu);
    if (device >= 0 && device < 64 && have[device]) {
        *d = accepted[device];
        return SSIMU2_OK;
    }
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->device = device;
    d->numa_node = -1;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        if (why) *why = std::string("no usable HIP device (hipGetDeviceCount: ") + hipGetErrorString(e) + ", " +
                        std::to_string(ndev) + " device(s), index " + std::to_string(device) + ")";
        return SSIMU2_ERR_NO_DEVICE;
    }
    hipDeviceProp_t pr;
    if ((e = hipGetDeviceProperties(&pr, device)) != hipSuccess) {
        if (why) *why = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return SSIMU2_ERR_HIP;
    }
    snprintf(d->arch, sizeof d->arch, "%s", pr.gcnArchName);
    snprintf(d->name, sizeof d->name, "%s", pr.name);
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess)
        snprintf(bus, sizeof bus, "%04x:%02x:%02x.0", pr.pciDomainID, pr.pciBusID, pr.pciDeviceID);
    for (char* q = bus; *q; ++q) *q = (char)tolower((unsigned char)*q);
    snprintf(d->pci_bus_id, sizeof d->pci_bus_id, "%s", bus);
    d->compute_units = pr.multiProcessorCount > 0 ? (uint32_t)pr.multiProcessorCount : 0;
    // LDS of one CU: the runtime reports it as maxSharedMemoryPerMultiProcessor; the per-workgroup limit
    // (sharedMemPerBlock) is the same number on gfx950 (a workgroup may take the whole 160 KB)
    d->lds_bytes_per_workgroup = (uint32_t)pr.sharedMemPerBlock;
    size_t per_cu = pr.maxSharedMemoryPerMultiProcessor;
    int attr = 0;
    if (hipDeviceGetAttribute(&attr, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && attr > 0 &&
        (size_t)attr > per_cu)
        per_cu = (size_t)attr;
    if (pr.sharedMemPerBlock > per_cu) per_cu = pr.sharedMemPerBlock;  // a workgroup's limit cannot exceed its CU's LDS
    d->lds_bytes_per_cu = (uint32_t)per_cu;
    d->wavefront_size = pr.warpSize > 0 ? (uint32_t)pr.warpSize : 0;
    d->hbm_bytes = (uint64_t)pr.totalGlobalMem;
    {
        char path[128];
        snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", d->pci_bus_id);
        if (FILE* f = fopen(path, "r")) {
            int node = -1;
            if (fscanf(f, "%d", &node) == 1) d->numa_node = node;
            fclose(f);
        }
    }
    (void)hipGetLastError();
    if (strncmp(d->arch, "gfx950", 6) != 0) {
        if (why) *why = std::string("device ") + std::to_string(device) + " is " + d->arch +
                        ", not gfx950: this library holds gfx950 (MI355X) code only";
        return SSIMU2_ERR_NO_DEVICE;
    }
    if (d->lds_bytes_per_cu < kMinLdsPerCu) {
        if (why) *why = std::string("device ") + std::to_string(device) + " (" + d->arch + ") reports " +
                        std::to_string(d->lds_bytes_per_cu) + " bytes of LDS per compute unit, LDS < 160 KB";
        return SSIMU2_ERR_NO_DEVICE;
    }
    if (d->wavefront_size != 64) {
        if (why) *why = std::string("device ") + std::to_string(device) + " runs wavefronts of " +
                        std::to_string(d->wavefront_size) + " lanes, the kernels are written for 64";
        return SSIMU2_ERR_NO_DEVICE;
    }
    d->usable = 1;
    if (device < 64) {
        accepted[device] = *d;
        have[device] = true;
    }
    return SSIMU2_OK;
}

int ssimu2_query_device(int device, ssimu2_device_info* out) {
    if (!out || out->struct_size != sizeof(ssimu2_device_info)) return SSIMU2_ERR_INVALID_ARG;
    if (ssimu2r::enabled()) return ssimu2r::query_device(device, ssimu2_version(), out, &g_create_error);  // the server's record
    ssimu2_device_info d;
    std::string why;
    const int rc = query_device_impl(device, &d, &why);
    if (rc == SSIMU2_ERR_NO_DEVICE && d.arch[0] == 0) {  // no such device at all
        g_create_error = why;
        return rc;
    }
    if (rc == SSIMU2_ERR_HIP) {
        g_create_error = why;
        return rc;
    }
    *out = d;  // a device of another kind is described too, with usable = 0
    return SSIMU2_OK;
}

int ssimu2_ctx_device_info(const ssimu2_ctx* c, ssimu2_device_info* out) {
    if (!c || !out || out->struct_size != sizeof(ssimu2_device_info)) return SSIMU2_ERR_INVALID_ARG;
    *out = c->dev;
    return SSIMU2_OK;
}

int ssimu2_host_alloc(ssimu2_ctx* c, size_t bytes, void** out_ptr) {
    REMOTE(c, host_alloc(c->remote, bytes, out_ptr));
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!out_ptr || bytes == 0) return c->fail(SSIMU2_ERR_INVALID_ARG, "ssimu2_host_alloc: null out_ptr or zero bytes");
    *out_ptr = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipError_t e = hipHostMalloc(out_ptr, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        *out_ptr = nullptr;
        (void)hipGetLastError();
        return c->fail(SSIMU2_ERR_OOM, "hipHostMalloc(pinned frame buffer)", e);
    }
    return SSIMU2_OK;
}

int ssimu2_host_free(ssimu2_ctx* c, void* ptr) {
    REMOTE(c, host_free(c->remote, ptr));
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!ptr) return SSIMU2_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipHostFree(ptr));
    return SSIMU2_OK;
}

static int ctx_create_impl(int device, void* hip_stream, ssimu2_ctx** out_ctx) {
    if (!out_ctx) return SSIMU2_ERR_INVALID_ARG;
    *out_ctx = nullptr;
    // capability check first (include/ssimu2_hip.h, SSIMU2_ERR_NO_DEVICE): a device index that exists, gfx950,
    // 160 KB of LDS per CU -- instead of a failure at the first launch on anything else
    ssimu2_device_info info;
    {
        std::string why;
        const int rc = query_device_impl(device, &info, &why);
        if (rc != SSIMU2_OK) {
            g_create_error = why;
            return rc;
        }
    }
    ssimu2_ctx* c = new (std::nothrow) ssimu2_ctx();
    if (!c) return SSIMU2_ERR_OOM;
    c->device = device;
    c->dev = info;
    c->rg_v_pad = rg_v_pad_bytes(info.lds_bytes_per_cu);
#define CREATE_TRY(call)                                                        \
    do {                                                                        \
        hipError_t e2 = (call);                                                 \
        if (e2 != hipSuccess) {                                                 \
            g_create_error = std::string(#call) + ": " + hipGetErrorString(e2); \
            ssimu2_ctx_destroy(c);                                              \
            return SSIMU2_ERR_HIP;                                              \
        }                                                                       \
    } while (0)
    CREATE_TRY(hipSetDevice(device));
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else if ((c->stream = pool_acquire(device)) != nullptr) {
        c->pool_stream = true;
    } else {
        CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    CREATE_TRY(hipEventCreate(&c->ev0));
    CREATE_TRY(hipEventCreate(&c->ev1));
    CREATE_TRY(hipMalloc(&c->d_result, 110 * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&c->h_result.p, 110 * sizeof(double), hipHostMallocDefault));
    c->h_result.cap = 110 * sizeof(double);
    {
        // The constant table lives in device memory of this module, one copy per device, shared
        // by every context on that device: upload it once per device (contexts may be created
        // from worker threads while other contexts' kernels are running).
        static std::mutex mu;
        static bool uploaded[64] = {false};
        std::lock_guard<std::mutex> lock(mu);
        if (device >= 64 || !uploaded[device]) {
            DevConst* k = new (std::nothrow) DevConst();
            if (!k) {
                ssimu2_ctx_destroy(c);
                return SSIMU2_ERR_OOM;
            }
            for (int i = 0; i < 256; ++i) {
                const double v = (double)i / 255.0;
                k->lut[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
            }
            gaussian_taps(1.5, k->taps, k->rg_n2, k->rg_d1);
            k->cbrt_bias = cbrt_repro<true>(kOpsinBias);
            memcpy(k->weights, kWeightsHost, sizeof kWeightsHost);
            hipError_t ec = hipMemcpyToSymbol(HIP_SYMBOL(c_k), k, sizeof(DevConst));
            delete k;
            CREATE_TRY(ec);
            if (device < 64) uploaded[device] = true;
        }
    }
#undef CREATE_TRY
    *out_ctx = c;
    return SSIMU2_OK;
}

void ssimu2_ctx_destroy(ssimu2_ctx* c) {
    if (!c) return;
    if (c->remote) {
        ssimu2r::destroy(c->remote);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    release_frame_groups(c);
    release(c->batch);
    release(c->tab);
    release(c->alpha_tab);
    (void)hipFree(c->d_result);
    release(c->h_result);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->pool_stream) pool_release(c->device, c->stream);
    delete c;
}

int ssimu2_wait(ssimu2_ctx* c, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_wait");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!c->pending) return c->fail(SSIMU2_ERR_INVALID_ARG, "ssimu2_wait: nothing enqueued");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->pending = false;
    if (out_score) *out_score = c->h_result.as<double>()[108];
    return SSIMU2_OK;
}

int ssimu2_enqueue_rgb8_device(ssimu2_ctx* c, const void* d_ref, const void* d_dist, uint32_t w,
                               uint32_t h) {
    REMOTE_REFUSE(c, "ssimu2_enqueue_rgb8_device");
    int rc = check_args(c, d_ref, d_dist, w, h);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    c->ref.drop();  // the lin_ref pyramid is overwritten
    return enqueue_score(c, (const uint8_t*)d_ref, (const uint8_t*)d_dist, w, h, false);
}

int ssimu2_score_rgb8_device(ssimu2_ctx* c, const void* d_ref, const void* d_dist, uint32_t w,
                             uint32_t h, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_rgb8_device");
    if (!out_score)
        return c ? c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score") : SSIMU2_ERR_INVALID_ARG;
    int rc = ssimu2_enqueue_rgb8_device(c, d_ref, d_dist, w, h);
    if (rc) return rc;
    return ssimu2_wait(c, out_score);
}

// FIR mode: the reference's positive-XYB planes and blur(ref*ref) at every scale from its scale 0 (`scale0`: the 8-bit
// frame, or with !scale0_u8 the linear planes of a 16-bit one) and its linear pyramid in d_lin_ref, already enqueued.
// `required` (16-bit references): a failed allocation is an error instead of a reference converted on every pass.
static int cache_reference_fir(ssimu2_ctx* c, const Pyramid& p, const void* scale0, bool scale0_u8, bool required) {
    // ... and its positive-XYB planes at every scale, so that the per-pass kernel skips the
    // LUT / opsin / cube-root work for the reference frame (same values, bit-identical scores).
    // A failed allocation of either plane set is not an error unless `required`: the search still works, the
    // reference is just converted (and all five planes blurred) on every pass.  A grow() that fails leaves the
    // buffer released and no sticky HIP error.
    const size_t bytes = (xyb_off(p, p.nscales) + 4) * sizeof(float);
    const char* what = "hipMalloc(cached reference planes)";
    (void)grow(c, c->cache.xyb, bytes, what);
    float* const xyb = c->cache.xyb.as<float>();
    if (xyb) launch_ref_xyb(c, p, scale0, scale0_u8, c->frame.lin_ref.as<float>(), xyb);
    // ... and blur(ref*ref) at every scale, which depends on the reference alone: the per-pass
    // kernel then blurs four planes instead of five (caching blur(ref) too was measured slower)
    if (xyb && c->cache_ref_blur) {
        (void)grow(c, c->cache.blur, bytes, what);
        if (c->cache.blur.p) {
            MarchPlan mp;
            FinalizeArgs fa;
            PlanSources src = score_sources(c, scale0, scale0, true);  // XYB planes in, blur(x*x) out
            src.lin_dist = src.lin_ref;                                // second frame unused
            const int blocks = build_plans(c, p, march_seg_rows, src, &mp, &fa, MARCH_OUT_PLANES);
            if (blocks > 0)
                launch(k_ref_blur, dim3(blocks), dim3(MARCH_THREADS), 0, c->stream, mp);
        }
    } else if (c->cache.blur.p) {  // the instrumented build's cache flag is off
        c->cache.blur.release();
    }
    if (required && !ref_cached(c))
        return c->fail(SSIMU2_ERR_OOM, "hipMalloc(cached planes of a 16-bit reference)");
    return SSIMU2_OK;
}

// The end of every ssimu2_set_reference*: everything of the reference is enqueued.
static int reference_set(ssimu2_ctx* c, uint32_t w, uint32_t h, bool hbd, int64_t bg) {
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // caller may free `ref` after return
    c->ref.set(w, h, hbd, bg);
    return SSIMU2_OK;
}

}  // extern "C"

// ---- the three shapes of a call that feeds frames, each once ----------------
// Every one of them, after the entry point's own argument checks: what can be refused without the device; the buffers
// (nothing enqueued yet that reads the caller's memory, so a failure returns as it is); then the copies and launches,
// from where leave() is the only way out.

// The pair score: `dist` against `ref`, two frames of one kind.
int ssimu2h::score_pair(ssimu2_ctx* c, const Feed& ref, const Feed& dist, uint32_t w, uint32_t h, double* out_score) {
    const bool recursive = c->blur_mode != SSIMU2_BLUR_FIR;
    int rc;
    if (recursive && (rc = rg_check_size(c, w, h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    c->ref.drop();  // the lin_ref pyramid is overwritten
    Fed r{}, d{};
    if ((recursive && (rc = rg_ensure(c, make_pyramid(w, h)))) || (rc = feed_reserve(c, ref, true, w, h, &r)) ||
        (rc = feed_reserve(c, dist, false, w, h, &d)))
        return rc;
    if (!(rc = feed_enqueue(c, ref, true, w, h, &r)) && !(rc = feed_enqueue(c, dist, false, w, h, &d)) &&
        !(rc = launch_score(c, w, h, &r, d)))
        rc = ssimu2_wait(c, out_score);
    return leave(c, rc);
}

// Set-reference: the frame, then everything that depends on the reference alone.
int ssimu2h::feed_reference(ssimu2_ctx* c, const Feed& ref, uint32_t w, uint32_t h) {
    const bool fir = c->blur_mode == SSIMU2_BLUR_FIR;
    int rc;
    if (!fir && (rc = rg_check_size(c, w, h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    const Pyramid p = make_pyramid(w, h);
    if (!fir && (rc = rg_ensure(c, p))) return rc;
    c->ref.drop();  // the lin_ref pyramid and the cached planes are overwritten
    Fed r{};
    if ((rc = feed_reserve(c, ref, true, w, h, &r))) return rc;
    if (!(rc = feed_enqueue(c, ref, true, w, h, &r))) {
        float* lin[1] = {c->frame.lin_ref.as<float>()};
        if (r.u8) note_lin0(c, 0, 0, w, h);
        if (!fir) {  // XYB planes, blur(x) and blur(x*x) by the published recursion
            rg_enqueue_reference(c, p, r.u8, r.u8 ? nullptr : &r.s16);
        } else if (r.u8) {  // the reference's linear pyramid, once per search, then the caches
            launch_pyramid(c, p, 1, &r.u8, lin);
            (void)cache_reference_fir(c, p, r.u8, true, false);  // not required: an 8-bit pass converts the reference
        } else {  // linear pyramid and scale-0 planes, then the same caches as an 8-bit reference's (required here)
            const Src16* src[1] = {&r.s16};
            float* lin0[1] = {c->hbd.lin0_ref.as<float>()};
            launch_pyramid16(c, p, 1, src, lin, lin0);
            if (p.nscales >= 1) note_lin0(c, 1, -1, w, h);
            rc = cache_reference_fir(c, p, lin0[0], false, true);
        }
        if (!rc) rc = reference_set(c, w, h, !r.u8, ref.bg);
        if (!rc) c->ref.lin0 = fir && !r.u8 && p.nscales >= 1;  // launch_pyramid16 above wrote hbd.lin0_ref
    }
    return leave(c, rc);
}

// The pass against the cached reference.
int ssimu2h::score_against(ssimu2_ctx* c, const Feed& dist, double* out_score) {
    const uint32_t w = c->ref.w, h = c->ref.h;
    HIP_TRY(c, hipSetDevice(c->device));
    Fed d{};
    int rc = pass_prepare(c, dist.top != 0);
    if (rc || (rc = feed_reserve(c, dist, false, w, h, &d))) return rc;
    if (!(rc = feed_enqueue(c, dist, false, w, h, &d)) && !(rc = launch_score(c, w, h, nullptr, d)))
        rc = ssimu2_wait(c, out_score);
    return leave(c, rc);
}

// What every against-reference call checks first, in this order; `pointers`: none of the call's pointers is null.
int ssimu2h::check_against(ssimu2_ctx* c, bool pointers) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!c->ref.have) return c->fail(SSIMU2_ERR_NO_REFERENCE, "no reference set");
    if (!pointers) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    return SSIMU2_OK;
}

// ---- the two shapes that add the error map (include/ssimu2_hip_map.h) --------
void (*ssimu2h::map_lin0_of_u8)(ssimu2_ctx*, const uint8_t*, const float*, size_t, float*) = nullptr;

// The pair score, then the map pass over the planes it left.
int ssimu2h::map_pair(ssimu2_ctx* c, const Feed& ref, const Feed& dist, uint32_t w, uint32_t h, float* out_map,
                      double* out_score) {
    const int rc = score_pair(c, ref, dist, w, h, out_score);
    return rc ? rc : map_pass(c, dist.top != 0, w, h, out_map);
}

// The pass against the cached reference, then the map pass.  What the FIR pass reads of the reference at scale 0:
// an 8-bit frame of u8 feeds against an 8-bit reference (ssimu2_error_map_against_reference's case, and its refusal
// of a 16-bit one: no 8-bit frame is kept of that); of u16 codes, hbd.lin0_ref, which feed_reference wrote of a
// 16-bit reference and nothing has touched since (ref.lin0: every call that regrows, rewrites or releases the plane
// drops the reference), and which is made here, once, of an 8-bit reference's frame.
int ssimu2h::map_against(ssimu2_ctx* c, const Feed& dist, float* out_map, double* out_score) {
    const bool hbd = dist.top != 0;
    if (!hbd && c->ref.hbd)
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "no error map of an 8-bit frame against a reference set from 16-bit samples");
    int rc = score_against(c, dist, out_score);
    if (rc) return rc;
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (hbd && c->blur_mode == SSIMU2_BLUR_FIR && !c->ref.lin0 && w >= 8 && h >= 8) {
        if (c->ref.hbd || !map_lin0_of_u8)  // neither happens: feed_reference sets lin0, the map unit the pointer
            return c->fail(SSIMU2_ERR_UNSUPPORTED, "error map: the reference's scale-0 linear planes are missing");
        const size_t n = (size_t)w * h;
        const float* tab8 = nullptr;
        if ((rc = grow(c, c->hbd.lin0_ref, n * 3 * sizeof(float), "hipMalloc(16-bit scale-0 planes)")) ||
            (rc = device_table(c, 256u, 255u, &tab8)))
            return rc;
        map_lin0_of_u8(c, c->frame.ref_u8.as<uint8_t>(), tab8, n, c->hbd.lin0_ref.as<float>());
        HIP_TRY(c, hipGetLastError());
        note_lin0(c, 1, -1, w, h);
        c->ref.lin0 = true;
    }
    return map_pass(c, hbd, w, h, out_map);
}

extern "C" {

int ssimu2_score_rgb8(ssimu2_ctx* c, const uint8_t* ref, const uint8_t* dist, uint32_t w,
                      uint32_t h, uint32_t channels, double* out_score) {
    REMOTE(c, score_rgb8(c->remote, ref, dist, w, h, channels, out_score));
    int rc = check_args(c, ref, dist, w, h);
    if (rc) return rc;
    if (channels != 3) return c->fail(SSIMU2_ERR_UNSUPPORTED, "channels must be 3");
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    return score_pair(c, tight8(ref, w), tight8(dist, w), w, h, out_score);
}

int ssimu2_set_reference(ssimu2_ctx* c, const uint8_t* ref, uint32_t w, uint32_t h) {
    REMOTE(c, set_reference(c->remote, ref, w, h));
    const int rc = check_args(c, ref, ref, w, h);
    return rc ? rc : feed_reference(c, tight8(ref, w), w, h);
}

int ssimu2_set_reference_device(ssimu2_ctx* c, const void* d_ref, uint32_t w, uint32_t h) {
    REMOTE_REFUSE(c, "ssimu2_set_reference_device");
    const int rc = check_args(c, d_ref, d_ref, w, h);
    return rc ? rc : feed_reference(c, tight8(d_ref, w, hipMemcpyDeviceToDevice), w, h);
}

int ssimu2_enqueue_against_reference_device(ssimu2_ctx* c, const void* d_dist) {
    REMOTE_REFUSE(c, "ssimu2_enqueue_against_reference_device");
    int rc = check_against(c, d_dist != nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return enqueue_score(c, c->frame.ref_u8.as<uint8_t>(), (const uint8_t*)d_dist, c->ref.w, c->ref.h, true);
}

int ssimu2_score_against_reference(ssimu2_ctx* c, const uint8_t* dist, double* out_score) {
    REMOTE(c, score_against_reference(c->remote, dist, out_score));
    const int rc = check_against(c, dist && out_score);
    return rc ? rc : score_against(c, tight8(dist, c->ref.w), out_score);
}

// Decoded 8-bit rows in `stage` -> the tight RGB8 frame `dst` (Feed::unpack of the call below).
static void unpack_rgb8(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, void* dst) {
    const uint32_t row_bytes = f.plane[0].row_bytes;
    if (f.ch == 4 && w % 4 == 0 && row_bytes % 4 == 0)
        launch(k_unpack_rgb<true>, dim3((w / 4 + 255) / 256, h), dim3(256), 0, c->stream, c->stage.as<uint8_t>(),
               row_bytes, f.ch, w, h, (uint8_t*)dst);
    else
        launch(k_unpack_rgb<false>, dim3((w + 255) / 256, h), dim3(256), 0, c->stream, c->stage.as<uint8_t>(),
               row_bytes, f.ch, w, h, (uint8_t*)dst);
}

int ssimu2_score_against_reference_strided(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes,
                                           uint32_t channels, double* out_score) {
    REMOTE(c, score_strided(c->remote, pixels, row_bytes, channels, out_score));
    int rc = check_against(c, pixels && out_score);
    if (rc) return rc;
    if (channels != 3 && channels != 4)
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "channels must be 3 (RGB) or 4 (RGBA)");
    const uint32_t w = c->ref.w;
    if ((uint64_t)row_bytes < (uint64_t)w * channels)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of pixels");
    if (channels == 3 && row_bytes == w * 3) return score_against(c, tight8(pixels, w), out_score);  // scorer's layout
    return score_against(c, staged1(pixels, row_bytes, channels, 1u, 0u, unpack_rgb8), out_score);
}

int ssimu2_error_map_rgb8(ssimu2_ctx* c, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h,
                          uint32_t channels, float* out_map, double* out_score) {
    REMOTE(c, error_map_rgb8(c->remote, ref, dist, w, h, channels, out_map, out_score));
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    int rc = ssimu2_score_rgb8(c, ref, dist, w, h, channels, out_score);
    if (rc) return rc;
    return map_pass(c, false, w, h, out_map);
}

int ssimu2_error_map_against_reference(ssimu2_ctx* c, const uint8_t* dist, float* out_map, double* out_score) {
    REMOTE(c, error_map_against_reference(c->remote, dist, out_map, out_score));
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    if (c->ref.have && c->ref.hbd)  // the map pass reads the reference's 8-bit frame
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "no error map against a reference set from 16-bit samples");
    int rc = ssimu2_score_against_reference(c, dist, out_score);
    if (rc) return rc;
    return map_pass(c, false, c->ref.w, c->ref.h, out_map);
}

// ---- 16-bit input ----------------------------------------------------------
int ssimu2_linear_table(uint32_t bit_depth, float* out) {
    if (!out) return SSIMU2_ERR_INVALID_ARG;
    if (bit_depth < 8 || bit_depth > 16) return SSIMU2_ERR_UNSUPPORTED;
    return copy_table(1u << bit_depth, (1u << bit_depth) - 1u, out);
}

int ssimu2_score_rgb16(ssimu2_ctx* c, const uint16_t* ref, const uint16_t* dist, uint32_t w, uint32_t h,
                       uint32_t channels, uint32_t bit_depth, double* out_score) {
    REMOTE(c, score_rgb16(c->remote, ref, dist, w, h, channels, bit_depth, out_score));
    int rc = check_args(c, ref, dist, w, h);
    if (rc) return rc;
    if ((rc = check16(c, ref, bit_depth)) || (rc = check16(c, dist, bit_depth))) return rc;
    if (channels != 3) return c->fail(SSIMU2_ERR_UNSUPPORTED, "channels must be 3");
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    return score_pair(c, tight16(ref, w, bit_depth), tight16(dist, w, bit_depth), w, h, out_score);
}

int ssimu2_set_reference_rgb16(ssimu2_ctx* c, const uint16_t* ref, uint32_t w, uint32_t h, uint32_t bit_depth) {
    REMOTE(c, set_reference_rgb16(c->remote, ref, w, h, bit_depth));
    int rc = check_args(c, ref, ref, w, h);
    if (rc || (rc = check16(c, ref, bit_depth))) return rc;
    return feed_reference(c, tight16(ref, w, bit_depth), w, h);
}

int ssimu2_score_against_reference_rgb16(ssimu2_ctx* c, const uint16_t* dist, uint32_t bit_depth, double* out_score) {
    REMOTE(c, score_against_reference_rgb16(c->remote, dist, bit_depth, out_score));
    int rc = check_against(c, out_score != nullptr);
    if (rc || (rc = check16(c, dist, bit_depth))) return rc;
    return score_against(c, tight16(dist, c->ref.w, bit_depth), out_score);
}

int ssimu2_score_against_reference_strided16(ssimu2_ctx* c, const uint16_t* pixels, uint32_t row_bytes,
                                             uint32_t channels, uint32_t bit_depth, double* out_score) {
    REMOTE(c, score_strided16(c->remote, pixels, row_bytes, channels, bit_depth, out_score));
    int rc = check_against(c, out_score != nullptr);
    if (rc || (rc = check16(c, pixels, bit_depth))) return rc;
    if (channels != 3 && channels != 4)
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "channels must be 3 (RGB) or 4 (RGBA)");
    if ((row_bytes & 1u) || (uint64_t)row_bytes < (uint64_t)c->ref.w * channels * 2)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes odd or smaller than one row of 16-bit pixels");
    // rows are read where they are, in `stage`: padding and alpha skipped by the front end
    return score_against(c, staged1(pixels, row_bytes, channels, 2u, (1u << bit_depth) - 1u, nullptr), out_score);
}

int ssimu2_last_averages(ssimu2_ctx* c, double* out, int* out_num_scales) {
    REMOTE(c, last_averages(c->remote, out, out_num_scales));
    if (!c || !out) return SSIMU2_ERR_INVALID_ARG;
    if (c->pending) {
        int rc = ssimu2_wait(c, nullptr);
        if (rc) return rc;
    }
    memcpy(out, c->h_result.p, 108 * sizeof(double));
    if (out_num_scales) *out_num_scales = (int)c->h_result.as<double>()[109];
    return SSIMU2_OK;
}

// ---- batch scoring ---------------------------------------------------------
int ssimu2_score_batch_rgb8_device(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t item_stride_bytes,
                                   uint32_t n, uint32_t w, uint32_t h, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_score_batch_rgb8_device");
    int rc = batch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, d_refs, d_dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    if ((uint64_t)item_stride_bytes < (uint64_t)w * h * 3)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "item_stride_bytes smaller than one frame");
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_run(c, (const uint8_t*)d_refs, (const uint8_t*)d_dists, item_stride_bytes, n, w, h, out_scores);
}

int ssimu2_score_batch_against_reference_device(ssimu2_ctx* c, const void* d_dists, size_t item_stride_bytes, uint32_t n,
                                                double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_score_batch_against_reference_device");
    int rc = batch_open(c, n, true);
    if (rc || n == 0) return rc;
    if (!d_dists || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((uint64_t)item_stride_bytes < (uint64_t)c->ref.w * c->ref.h * 3)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "item_stride_bytes smaller than one frame");
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_run(c, nullptr, (const uint8_t*)d_dists, item_stride_bytes, n, c->ref.w, c->ref.h, out_scores);
}

int ssimu2_score_batch_rgb8(ssimu2_ctx* c, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n, uint32_t w,
                            uint32_t h, double* out_scores) {
    REMOTE(c, score_batch_rgb8(c->remote, refs, dists, n, w, h, out_scores));
    int rc = batch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, refs, dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    for (uint32_t i = 0; i < n; ++i)
        if (!refs[i] || !dists[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * 3, stride = (bytes + 15) & ~(size_t)15;
    if (!(rc = batch_stage(c, c->batch.u8_ref, refs, n, bytes, stride)) &&
        !(rc = batch_stage(c, c->batch.u8_dist, dists, n, bytes, stride)))
        rc = batch_run(c, c->batch.u8_ref.as<uint8_t>(), c->batch.u8_dist.as<uint8_t>(), stride, n, w, h, out_scores);
    return leave(c, rc);
}

int ssimu2_score_batch_against_reference(ssimu2_ctx* c, const uint8_t* const* dists, uint32_t n, double* out_scores) {
    REMOTE(c, score_batch_against_reference(c->remote, dists, n, out_scores));
    int rc = batch_open(c, n, true);
    if (rc || n == 0) return rc;
    if (!dists || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    for (uint32_t i = 0; i < n; ++i)
        if (!dists[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->ref.w * c->ref.h * 3, stride = (bytes + 15) & ~(size_t)15;
    if (!(rc = batch_stage(c, c->batch.u8_dist, dists, n, bytes, stride)))
        rc = batch_run(c, nullptr, c->batch.u8_dist.as<uint8_t>(), stride, n, c->ref.w, c->ref.h, out_scores);
    return leave(c, rc);
}

int ssimu2_last_batch_averages(ssimu2_ctx* c, uint32_t item, double* out, int* out_num_scales) {
    REMOTE(c, last_batch_averages(c->remote, item, out, out_num_scales));
    if (!c || !out) return SSIMU2_ERR_INVALID_ARG;
    if (item >= c->batch_n) return c->fail(SSIMU2_ERR_INVALID_ARG, "ssimu2_last_batch_averages: no such item in the last batch");
    const double* r = c->batch.result.as<double>() + (size_t)item * kResultDoubles;
    memcpy(out, r, 108 * sizeof(double));
    if (out_num_scales) *out_num_scales = (int)r[109];
    return SSIMU2_OK;
}

}  // extern "C"
