// What a front end of the MI355X SSIMULACRA2 scorer may use of its host code: the interface between ssimu2_hip.hip
// (which defines everything declared here but the front ends' own feed builders, marked below) and the translation
// units that add an input form -- ssimu2_ext.hip (RGBA), ssimu2_yuv.hip (YUV), ssimu2_chroma.hip (4:2:2 and 4:2:0
// YUV), ssimu2_yuva.hip (YUV with an alpha plane) -- or a call over those forms -- ssimu2_map.hip (error maps of 16-bit, RGBA and YUV frames),
// ssimu2_rbatch.hip (batches in every blur mode), ssimu2_hbatch.hip (16-bit and YUV batches), ssimu2_abatch.hip (RGBA
// and YUV-with-alpha batches).  Private to oavif_amd/csrc: nothing here is exported,
// and a caller sees include/*.h only.
//
// A front end turns a caller's frame into a Feed -- where its rows are, how they get onto the device, what kernel of
// the front end's own makes tight u16 codes of them (Feed::unpack) and through which table the scorer reads those --
// and hands it to one of the three shapes of a call: score_pair, feed_reference, score_against, or to the two that
// add the error map (map_pair, map_against).  Everything else of ssimu2_hip.hip (plans, pyramids, the recursive path,
// batch, the map pass, the stream pool) is that unit's own.
//
// No kernel and no __constant__ lives here or in anything this header includes (ssimu2_kernels.h and
// ssimu2_recursive.h are ssimu2_hip.hip's alone): the units that include it are linked into one library, where a
// second definition of a kernel is a clash and a second c_k a constant block nobody uploads.
#pragma once

// ssimu2_ctx ends in fields that only the instrumented build has, so every unit of a library must agree on the macro.
// The instrumented library is one unit, ssimu2_instrument.hip, which includes ssimu2_hip.hip: nothing else may see it.
#if defined(SSIMU2_INSTRUMENTED_BUILD) && !defined(SSIMU2_CORE_UNIT)
#error "ssimu2_host.h under SSIMU2_INSTRUMENTED_BUILD: only ssimu2_instrument.hip (through ssimu2_hip.hip) is built with it"
#endif

#include <hip/hip_runtime.h>
#ifdef SSIMU2_INSTRUMENTED_BUILD
#include <hip/hip_ext.h>
#endif

#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/ssimu2_hip.h"
#include "remote_client.h"

namespace ssimu2h {

// One buffer of a context: device memory, or (`host`) page-locked host memory that a kernel writes.  `cap` is in
// bytes, always; p is null exactly when cap is 0.  grow() is the one place that allocates.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool host = false;
    template <class T>
    T* as() const { return (T*)p; }
    void release() {
        (void)(host ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};

}  // namespace ssimu2h

struct ssimu2_yuv_frame;   // include/ssimu2_hip_yuv.h
struct ssimu2_yuva_frame;  // include/ssimu2_hip_yuva.h

struct ssimu2_ctx {
    using DevBuf = ssimu2h::DevBuf;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;   // created here, destroyed with the ctx
    bool pool_stream = false;  // borrowed from the process-wide set of streams on distinct hardware queues
    std::string err;
    // set: the context lives in a scoring service (OAVIF_SCORER_SOCKET at ssimu2_ctx_create, remote_client.h); nothing
    // below is used then, and every entry point hands over to it on its first line (REMOTE)
    ssimu2r::Remote* remote = nullptr;

    int blur_mode = SSIMU2_BLUR_FIR;
    ssimu2_device_info dev{};  // what ctx_create saw of the device (and checked: gfx950, 160 KB of LDS per CU)

    // The buffers, grouped by who releases them: the rows of DESIGN.md section 3, "Which call touches which buffer".
    // A group is a struct of DevBuf members and nothing else, so that release(group) finds every one of them.
    // Every group from `frame` to `hbd` is released when the frame buffers regrow (release_frame_groups).
    // frame: ensure_capacity grows all five or none
    struct {
        DevBuf ref_u8, dist_u8;    // interleaved RGB8
        DevBuf lin_ref, lin_dist;  // fp32, scales 1..5 packed
        DevBuf partials;           // fp64 [scale][18][workgroups]
    } frame;
    // cache: cache_reference_fir, for a reference set in FIR mode
    struct {
        DevBuf xyb;   // positive-XYB planes of the reference, all scales
        DevBuf blur;  // blur(ref*ref) planes, all scales (null = not cached)
    } cache;
    // stage: feed_reserve, for a frame whose rows are not the scorer's (the _strided, _strided16, RGBA and YUV calls)
    DevBuf stage;  // decoded avifRGBImage as uploaded (RGBA / padded rows)
    // rg: rg_ensure, SSIMU2_BLUR_RECURSIVE modes only (ssimu2_recursive.h); also released by ssimu2_ctx_set_blur(FIR)
    struct {
        DevBuf planes;  // fp32, every scale packed: XYB planes of both frames [3], the reference's cached mu1 / s11
                        // planes [6], the horizontal pass of a pass's planes [9]
        DevBuf part;    // fp64 [scale][18][column groups]
        DevBuf dbg;     // instrumented builds: 15 + 15 raw fp32 planes of scale rg_dbg_scale
    } rg;
    unsigned* d_rg_q = nullptr;  // job cursor of the persistent vertical pass (RgPlan::q, 4 words); released with `rg`
    int num_cus = 0;             // workgroups of that kernel: one per CU
    unsigned rg_v_pad = 0;       // unused dynamic LDS of k_rg_v's launch: rg_v_pad_bytes(dev.lds_bytes_per_cu)
    // map: map_ensure, by the first ssimu2_error_map_* call
    struct {
        DevBuf dens;  // fp32 per-(scale, channel) density planes [scale][3][h_s][w_s]
        DevBuf out;   // the full-resolution fp32 map [h][w]
    } map;
    // hbd: the first 16-bit call (ssimu2_*_rgb16 / _strided16)
    struct {
        DevBuf ref16, dist16;        // the tight u16 frames
        DevBuf lin0_ref, lin0_dist;  // FIR: the frames' scale-0 linear planes, fp32 [3][h][w]
    } hbd;
    // tab: device_table; released by ssimu2_ctx_destroy only.  The sRGB -> linear tables of depths 8..16: depth d at
    // float offset 2^d - 256, uploaded by the first call at that depth
    DevBuf tab;
    // alpha: device_table, by the first RGBA call (the extension library's: ssimu2_ext.hip, include/ssimu2_hip_ext.h;
    // nothing in the product library feeds RGBA); released by ssimu2_ctx_destroy only.  The table of the 65,026
    // composite codes
    DevBuf alpha_tab;
    uint32_t tab_ready = 0;  // bit d: the depth-d table is in `tab`; bit 0: the composite table is in `alpha_tab`
    // batch: batch_run / batch_stage (ssimu2_score_batch_*), each buffer when too small; released by ssimu2_ctx_destroy
    // only.  Scratch of its own, so a batch leaves the single-score buffers and a cached reference alone: the staged
    // 8-bit frames of the host-pointer forms, the linear pyramids (scales 1..5) and partial sums of every item, and the
    // page-locked result block k_finalize_batch writes (110 doubles per item).  rg_planes / rg_part: rbatch_run, by
    // the first batch in a recursive mode -- every item's planes, then one dump row; the job
    // cursor's four words, then every item's partial sums.  h16_ref / h16_dist / yuv_planes: the calls of
    // include/ssimu2_hip_hbatch.h -- the staged 16-bit frames of the host-pointer forms or the
    // codes of a YUV batch, and the staged planes of a YUV batch.  The calls of include/ssimu2_hip_abatch.h (DESIGN.md
    // section 20) add none: they stage planes and RGBA rows in yuv_planes and make their codes in h16_dist
    struct {
        DevBuf u8_ref, u8_dist, lin_ref, lin_dist, part;
        DevBuf rg_planes, rg_part;
        DevBuf h16_ref, h16_dist, yuv_planes;
        DevBuf result{nullptr, 0, true};
    } batch;
    uint32_t batch_n = 0;  // items of the last finished batch (ssimu2_last_batch_averages)
    // result: ssimu2_ctx_create; ssimu2_ctx_destroy
    double* d_result = nullptr;         // 110 doubles in device memory: the stage timing of the instrumented build only
    DevBuf h_result{nullptr, 0, true};  // page-locked host memory k_finalize writes the result into (110 doubles)

    // The cached reference: set by reference_set, dropped where its storage is released or overwritten
    struct {
        bool have = false, hbd = false;  // hbd: set from 16-bit samples (its 8-bit frame buffer is not it)
        bool lin0 = false;  // FIR: hbd.lin0_ref holds its scale-0 linear planes (feed_reference of 16-bit samples, or
                            // map_against, which makes them of an 8-bit reference's frame on its first call)
        uint32_t w = 0, h = 0;
        int64_t bg = -1;  // 0xRRGGBB the reference was composited over (ssimu2_set_reference_rgba8); -1: none recorded
        void drop() { have = hbd = lin0 = false, w = h = 0, bg = -1; }
        void set(uint32_t w_, uint32_t h_, bool hbd_, int64_t bg_) {
            have = true, hbd = hbd_, lin0 = false, w = w_, h = h_, bg = bg_;
        }
    } ref;
    bool pending = false;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // measurement builds only (ssimu2_instrument.hip); always 0 / true in the product library
    int seg_rows_override = 0;
    int seg_rows_tail_override = 0;
    int batch_seg_override = 0;  // scale-0 rows of a batch item: 0 = the rule, -1 = the single-score rule, 8..160 fixed
    bool cache_ref_blur = true;
    int rg_dbg_scale = -1;  // recursive mode: keep that scale's 15 raw planes (after each pass) downloadable
#ifdef SSIMU2_INSTRUMENTED_BUILD
    // the frame size whose scale-0 planes hbd.lin0_ref / hbd.lin0_dist hold for the last score or reference (0: none;
    // for ssimu2_debug_download at scale 0)
    uint32_t lin0_ref_w = 0, lin0_ref_h = 0, lin0_dist_w = 0, lin0_dist_h = 0;
    int last_march = 0;  // SSIMU2_MARCH_* of the last score or batch (ssimu2_instr_last_march)
#endif

    int fail(int code, const char* what, hipError_t e = hipSuccess) {
        char buf[256];
        if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else snprintf(buf, sizeof buf, "%s", what);
        err = buf;
        return code;
    }
};

#define REMOTE(c, call) \
    if ((c) && (c)->remote) return ssimu2r::call
#define REMOTE_REFUSE(c, name) REMOTE(c, unsupported((c)->remote, name))

#define HIP_TRY(ctx, call)                                                   \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return (ctx)->fail(SSIMU2_ERR_HIP, #call, e_); \
    } while (0)

namespace ssimu2h {

// Every kernel of a score goes through launch().  Product build: hipLaunchKernelGGL, nothing else.  Instrumented build
// (ssimu2_instrument.hip): while a timing scope is open on the calling thread the same launch is made with
// hipExtLaunchKernelGGL and a start / stop event pair, so the duration of each kernel comes from its own dispatch packet
// (what rocprofv3's kernel trace reads) with no marker or barrier packet added between the launches of a score.
template <class T>
struct arg_of { using type = T; };
#ifdef SSIMU2_INSTRUMENTED_BUILD
struct LaunchTimer {
    hipEvent_t* ev;  // cap events: launch k of the scope uses ev[2k] (start) and ev[2k + 1] (stop)
    int n, cap;
};
inline thread_local LaunchTimer* g_launch_timer = nullptr;
#endif
template <typename... KArgs>
inline void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, unsigned lds, hipStream_t stream,
                   typename arg_of<KArgs>::type... args) {
#ifdef SSIMU2_INSTRUMENTED_BUILD
    if (LaunchTimer* t = g_launch_timer) {
        if (t->n + 2 <= t->cap) {
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, t->ev[t->n], t->ev[t->n + 1], 0, args...);
            t->n += 2;
            return;
        }
    }
#endif
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

// ---- 16-bit input ----------------------------------------------------------
// One 16-bit frame on the device: rows `pitch` bytes apart, `ch` = 3 (RGB) or 4 (RGBA) samples per pixel, read through
// the table of its depth.
struct Src16 {
    const void* px;
    uint32_t pitch, ch;
    const float* tab;
    uint32_t maxv;
};

// A frame where the front end reads it: an 8-bit RGB frame (`u8`), or with `u8` null 16-bit codes (`s16`).
struct Fed {
    const uint8_t* u8;
    Src16 s16;
};

// ---- a caller's frame onto the device ("One path for a frame") ---------------
// How one frame of a call gets onto the device, for either slot of the context (the reference's or the distorted
// frame's), and how the front end reads it there.
struct Plane {
    const void* px;      // the caller's rows
    uint32_t row_bytes;  // bytes between them
    uint32_t w = 0, h = 0;  // its own size in pixels where it is not the frame's (subsampled chroma); 0 = the frame's
};
struct Feed {
    // The caller's frame: one plane of interleaved pixels, or up to four planes of one sample per pixel -- Y, or Y, U
    // and V, then an alpha plane if there is one (`unpack` makes the pixels of them); all `nplanes` of them of one
    // layout (`ch`, `sample`) and in one place (`kind`)
    Plane plane[4];
    uint32_t nplanes;
    hipMemcpyKind kind;  // where they are: host memory, or an 8-bit frame already on the device
    uint32_t ch;         // samples per pixel there: 3, or 4 with the fourth skipped or composited away; 1 in a planar frame
    uint32_t sample;     // bytes per sample there: 1 or 2
    // 0: the front end reads an 8-bit RGB frame.  Else it reads u16 codes 0..top through the table of top + 1 entries:
    // 2^d - 1 for samples of depth d, 65025 for composite codes
    uint32_t top;
    // The rows go into the slot's tight frame as they are (`staged` false: they are tight RGB), or into `stage`.  From
    // there `unpack` launches what makes the slot's tight frame `dst` of them; with none the front end reads them in
    // `stage`, pitch, fourth sample and all (16-bit samples only)
    bool staged;
    void (*unpack)(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, void* dst);
    int64_t bg;  // 0xRRGGBB the unpacking composites over, which a reference keeps (ref.bg); -1: none
    const void* aux = nullptr;  // what else `unpack` needs to know, the entry point's own; alive for the call
};

// A frame of one plane in host memory, staged: rows `row_bytes` apart of `ch` samples of `sample` bytes per pixel.
Feed staged1(const void* px, uint32_t row_bytes, uint32_t ch, uint32_t sample, uint32_t top,
             void (*unpack)(ssimu2_ctx*, const Feed&, uint32_t, uint32_t, void*), int64_t bg = -1);
// Where plane `p` lies in `stage`: the planes back to back, each start 16-byte aligned (plane 0 at 0).
size_t plane_off(const Feed& f, uint32_t p, uint32_t w, uint32_t h);

// Feeding a frame in two halves (every feed_reserve of a call before its first feed_enqueue), and the one way out of a
// call from its first copy out of the caller's memory onwards.  The three shapes below do all of it; a front end calls
// these itself only for a diagnostic (feed_codes).
int feed_reserve(ssimu2_ctx* c, const Feed& f, bool ref, uint32_t w, uint32_t h, Fed* fed);
int feed_enqueue(ssimu2_ctx* c, const Feed& f, bool ref, uint32_t w, uint32_t h, Fed* fed);
int leave(ssimu2_ctx* c, int rc);
// The diagnostics of the front ends (ssimu2_composite_rgba8, ssimu2_convert_yuv): feed one frame of u16 codes and
// download its w * h * 3 codes into `out_codes`; `what` names the entry point in a HIP error.
int feed_codes(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, uint16_t* out_codes, const char* what);

// Argument checks: of a call that names a frame size (the ctx may be null); of an against-reference call, in this
// order: the ctx, the reference, `pointers` (none of the call's pointers is null).
int check_args(ssimu2_ctx* c, const void* a, const void* b, uint32_t w, uint32_t h);
int check_against(ssimu2_ctx* c, bool pointers);

// The table of the `n` codes 0..top as the exported functions hand it out.
int copy_table(uint32_t n, uint32_t top, float* out);

// The three shapes of a call that feeds frames, after the entry point's own argument checks: the
// pair score of two frames of one kind, set-reference, the pass against the cached reference.
int score_pair(ssimu2_ctx* c, const Feed& ref, const Feed& dist, uint32_t w, uint32_t h, double* out_score);
int feed_reference(ssimu2_ctx* c, const Feed& ref, uint32_t w, uint32_t h);
int score_against(ssimu2_ctx* c, const Feed& dist, double* out_score);

// ---- error maps of any feed (include/ssimu2_hip_map.h) ----------------------
// score_pair / score_against, then the map pass over what that score left in place: the w * h floats of section 9's
// map into `out_map`.  One path for every kind of frame; out_map and out_score are not null.
int map_pair(ssimu2_ctx* c, const Feed& ref, const Feed& dist, uint32_t w, uint32_t h, float* out_map, double* out_score);
int map_against(ssimu2_ctx* c, const Feed& dist, float* out_map, double* out_score);
// FIR, a frame of u16 codes against a reference set from 8-bit samples: the marching map reads scale 0 of both frames
// as linear planes, which such a reference does not have.  map_against makes them once per reference, of its retained
// 8-bit frame through the 8-bit table `tab` (entry 257 u of the depth-16 table is that entry u: the planes of the
// codes 257 u), with this launch: n pixels of interleaved RGB8 -> fp32 [3][n].  The kernel is ssimu2_map.hip's, which
// sets the pointer when its library is loaded; null in a library without that unit, where nothing calls map_against.
extern void (*map_lin0_of_u8)(ssimu2_ctx* c, const uint8_t* rgb8, const float* tab, size_t n, float* lin0);

// ---- batches in every blur mode (include/ssimu2_hip_rbatch.h) ---------------
// What ssimu2_rbatch.hip's four calls are made of.  rbatch_open: what every batch call refuses first, used as
// `if (rc || n == 0) return rc;` -- a null context, an empty batch (SSIMU2_OK), a missing reference, too many items;
// no blur mode is refused.  rbatch_check_size: the recursive modes' limit per item (nothing in FIR).  rbatch_stage: n
// host frames of `bytes` bytes into the batch's own staging buffer of the reference or distorted side, `stride` bytes
// apart, on the context stream; *d_frames is where they lie.  rbatch_run: n device-resident items of w x h, d_dists +
// i * stride0 against d_refs + i * stride0 or (d_refs null) against the cached reference, in the context's blur mode
// -- FIR: the batch of ssimu2_score_batch_*; recursive: one conversion, one launch per pass, one final reduction
// whatever n is.  Blocking; fills the batch result block, so ssimu2_last_batch_averages serves it.
int rbatch_open(ssimu2_ctx* c, uint32_t n, bool against_reference);
int rbatch_check_size(ssimu2_ctx* c, uint32_t w, uint32_t h);
int rbatch_stage(ssimu2_ctx* c, bool ref, const uint8_t* const* frames, uint32_t n, size_t bytes, size_t stride,
                 const uint8_t** d_frames);
int rbatch_run(ssimu2_ctx* c, const uint8_t* d_refs, const uint8_t* d_dists, size_t stride0, uint32_t n, uint32_t w,
               uint32_t h, double* out_scores);

// ---- 16-bit and YUV batches (include/ssimu2_hip_hbatch.h) -------------------
// What ssimu2_hbatch.hip's calls are made of, beside rbatch_open and rbatch_check_size.  hbatch_buffer: one of the
// batch group's three buffers of that unit -- 0: the references' 16-bit frames, 1: the distorted side's frames or the
// codes of a YUV batch, 2: the staged planes of a YUV batch -- holding `bytes` bytes and 16 of slack.  hbatch_table:
// the device table of `depth`, as a single 16-bit call reads it.  hbatch_run, recursive modes only: n items of tight
// u16 RGB frames of w x h on the device, d_dists + i * stride0 against d_refs + i * stride0 or (d_refs null) against
// the cached reference, read through `tab` with samples above 2^depth - 1 clamped; blocking, fills the batch result
// block like rbatch_run.  hbatch_check_launch: the "fewer items per call" refusal hbatch_run would make; every form
// makes it itself first, before it allocates (the depth's table, the staging buffers) or copies anything.
int hbatch_buffer(ssimu2_ctx* c, int which, size_t bytes, uint8_t** d_buf);
int hbatch_table(ssimu2_ctx* c, uint32_t depth, const float** tab);
int hbatch_check_launch(ssimu2_ctx* c, uint32_t n, uint32_t w, uint32_t h, bool against_reference);
int hbatch_run(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t stride0, uint32_t n, uint32_t w, uint32_t h,
               const float* tab, uint32_t depth, double* out_scores);

// ---- RGBA and YUV-with-alpha batches (include/ssimu2_hip_abatch.h) ----------
// What ssimu2_abatch.hip's calls add to the functions above.  abatch_run is hbatch_run for frames of composite codes:
// the same rbatch_recursive, the items read through the context's composite table T (uploaded by the first call that
// needs it, as a single RGBA call does) with codes above 65025 clamped.  hbatch_buffer's buffers serve these calls too.
int abatch_run(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t stride0, uint32_t n, uint32_t w, uint32_t h,
               double* out_scores);

// ---- what the front ends build their feeds with, for the units above them -------------------------
// A tight frame of u16 samples of depth `bit_depth` in host memory, and the 16-bit calls' argument checks (the ctx is
// not null).  Defined in ssimu2_hip.hip.
Feed tight16(const void* px, uint32_t w, uint32_t bit_depth);
int check16(ssimu2_ctx* c, const void* px, uint32_t bit_depth);
// RGBA (defined in ssimu2_ext.hip; in the libraries that link it): the argument checks of the calls that name a frame
// size (the ctx may be null), and one RGBA frame in host memory composited over `bg`.
int check_rgba(ssimu2_ctx* c, const void* a, const void* b, uint32_t row_bytes_a, uint32_t row_bytes_b, uint32_t w,
               uint32_t h, uint32_t background_rgb);
Feed rgba8_feed(const uint8_t* pixels, uint32_t row_bytes, uint32_t bg);
int rgba_no_background(ssimu2_ctx* c);  // the refusal of an against-reference call whose reference recorded no background
// YUV (defined in ssimu2_yuv.hip; in the libraries that link it): the constants of one conversion, formed on the host
// in fp32 exactly as include/ssimu2_hip_yuv.h writes them; what a YUV Feed's unpacking needs beyond the planes
// (Feed::aux, which outlives the call); the argument checks of one frame for a call of `w` columns (the ctx is not
// null); the frame's Feed.
struct YuvK {
    float bias_y, range_y, bias_uv, range_uv;
    float r_cr, b_cb;    // 2 (1 - kr), 2 (1 - kb)
    float g_cr, g_cb;    // kr (1 - kr), kb (1 - kb)
    float kg;
    float top;           // (float)(2^rgb_depth - 1)
    uint32_t max_code;   // m = 2^depth - 1: a 16-bit sample above it is read as m
};
struct YuvAux {
    YuvK k;
    bool mono;
};
int check_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* f, uint32_t w, uint32_t rgb_depth);
Feed yuv_feed(const ssimu2_yuv_frame& f, uint32_t rgb_depth, YuvAux* aux);
// Subsampled YUV (defined in ssimu2_chroma.hip; in the libraries that link it): what the unpacking of a frame of any of
// the four formats needs beyond the planes -- `yuv` comes first: a 4:4:4 or 4:0:0 frame's Feed::aux points at it, for
// yuv_feed's own unpacking --, the argument checks of one such frame (the ctx is not null), and its Feed for a w x h
// call, planes 1 and 2 with their own size.
struct ChromaAux {
    YuvAux yuv;
    bool vertical, bilinear;  // 4:2:0; the bilinear blend (both false for a 4:4:4 or 4:0:0 frame)
};
int check_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* f, uint32_t w, uint32_t rgb_depth, uint32_t upsampling);
Feed chroma_feed(const ssimu2_yuv_frame& f, uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t upsampling, ChromaAux* aux);

// YUV with an alpha plane (defined in ssimu2_yuva.hip; in the libraries that link it): the argument checks of one such
// frame for a call of `w` columns (the ctx is not null) -- check_chroma's, premultiplied alpha, the alpha plane's pitch
// and alignment --, check_rgba's background rule on its own, and the refusal of an against-reference call whose
// reference recorded no background.
int check_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* f, uint32_t w, uint32_t rgb_depth, uint32_t upsampling);
int check_background(ssimu2_ctx* c, uint32_t background_rgb);
int no_background(ssimu2_ctx* c);

}  // namespace ssimu2h
