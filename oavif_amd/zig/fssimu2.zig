//! Drop-in `fssimu2` module for oavif that scores on an MI355X through liboavif_hip.so.
//!
//! oavif imports the scorer by module name and calls it at exactly one place:
//!
//!     src/tq.zig:3    const fssimu2 = @import("fssimu2");
//!     src/tq.zig:37   return try fssimu2.computeSsimu2(allocator, e.rgb, decoded_rgb, e.w, e.h, 3, null);
//!
//! Point the "fssimu2" import of build.zig (build.zig:30-33,65) at this file and link
//! liboavif_hip.so (INTEGRATION.md); src/tq.zig needs no edit.
//!
//! NOT COMPILED IN THIS REPO'S CI: the build container has no Zig toolchain.  The C ABI it
//! binds (include/ssimu2_hip.h) is exercised by tests/ through ctypes instead.  The exact
//! types of fssimu2 0.1.1's 6th and 7th parameters are not visible from the reference
//! (its source is absent); they are declared here as what the call site passes: a
//! comptime-known integer and `null`.

const std = @import("std");

pub const Error = error{
    InvalidArgument, // SSIMU2_ERR_INVALID_ARG  (-1)
    UnsupportedChannels, // SSIMU2_ERR_UNSUPPORTED (-2)
    OutOfMemory, // SSIMU2_ERR_OOM          (-3)
    HipFailure, // SSIMU2_ERR_HIP          (-4)
    NoReference, // SSIMU2_ERR_NO_REFERENCE (-5)
    NoDevice, // SSIMU2_ERR_NO_DEVICE    (-6)
    Unknown,
};

const Ctx = opaque {};

extern fn ssimu2_ctx_create(device: c_int, hip_stream: ?*anyopaque, out_ctx: *?*Ctx) c_int;
extern fn ssimu2_prefetch(device: c_int) c_int;
extern fn ssimu2_prefetch_join(device: c_int) c_int;
extern fn ssimu2_ctx_destroy(ctx: ?*Ctx) void;
extern fn ssimu2_ctx_set_blur(ctx: ?*Ctx, mode: c_int) c_int;
extern fn ssimu2_last_error(ctx: ?*const Ctx) [*:0]const u8;
extern fn ssimu2_score_rgb8(ctx: ?*Ctx, ref: [*]const u8, dist: [*]const u8, w: u32, h: u32, channels: u32, out_score: *f64) c_int;
extern fn ssimu2_set_reference(ctx: ?*Ctx, ref: [*]const u8, w: u32, h: u32) c_int;
extern fn ssimu2_score_against_reference(ctx: ?*Ctx, dist: [*]const u8, out_score: *f64) c_int;
extern fn ssimu2_error_map_rgb8(ctx: ?*Ctx, ref: [*]const u8, dist: [*]const u8, w: u32, h: u32, channels: u32, out_map: [*]f32, out_score: *f64) c_int;
extern fn ssimu2_error_map_against_reference(ctx: ?*Ctx, dist: [*]const u8, out_map: [*]f32, out_score: *f64) c_int;
extern fn ssimu2_score_against_reference_strided(ctx: ?*Ctx, pixels: [*]const u8, row_bytes: u32, channels: u32, out_score: *f64) c_int;
extern fn ssimu2_score_rgb16(ctx: ?*Ctx, ref: [*]const u16, dist: [*]const u16, w: u32, h: u32, channels: u32, bit_depth: u32, out_score: *f64) c_int;
extern fn ssimu2_score_against_reference_strided16(ctx: ?*Ctx, pixels: [*]const u16, row_bytes: u32, channels: u32, bit_depth: u32, out_score: *f64) c_int;
extern fn ssimu2_score_batch_rgb8(ctx: ?*Ctx, refs: [*]const [*]const u8, dists: [*]const [*]const u8, n: u32, w: u32, h: u32, out_scores: [*]f64) c_int;
extern fn ssimu2_score_batch_against_reference(ctx: ?*Ctx, dists: [*]const [*]const u8, n: u32, out_scores: [*]f64) c_int;
extern fn ssimu2_host_alloc(ctx: ?*Ctx, bytes: usize, out_ptr: *?*anyopaque) c_int;
extern fn ssimu2_host_free(ctx: ?*Ctx, ptr: ?*anyopaque) c_int;

/// HIP device the process-wide scorer context binds to (set before the first call; the
/// batch driver gives every worker process its own device).
pub var device: c_int = 0;

/// oavif scores every pass of a search against the same `e.rgb` slice (main.zig:86,
/// tq.zig:37).  When true, a reference slice with the same pointer, length, dimensions and
/// content fingerprint (4 KiB of it: 64 runs of 64 bytes spread over the frame) as the previous
/// call is uploaded (and its caches built) only once.  Set to false -- or call invalidateReference() -- if the caller rewrites
/// the reference buffer in place between calls; hosts that process several images per process
/// should call invalidateReference() when an image's `e.rgb` is freed (INTEGRATION.md 2a).
pub var cache_reference: bool = true;

/// Which blur the scorer evaluates (include/ssimu2_hip.h, ssimu2_ctx_set_blur):
///   `.recursive`  DEFAULT of this shim (the search path) since round 4: the published recursive
///                 Gaussian operation for operation (libjxl's scalar order; planes bit-identical to the
///                 CPU checker's), 0.37 ms per 4K pass with the reference cached -- 0.1 % of a pass's
///                 encode + decode;
///   `.recursive_fma`  the same recursion with its multiply-subtract fused (what a compiler targeting
///                 an FMA unit makes of the published code);
///   `.fir`        the THROUGHPUT mode (what the benchmarks measure, what a context starts in at the
///                 C ABI): the recursion's exact 9-tap impulse response in fused kernels, 0.15 ms.
/// Why `.recursive`: fssimu2's source was not available where this shim was written, so which fp32
/// evaluation of the blur it follows is unknown.  The modes differ by the recursion's own rounding
/// noise -- median 0.02 points on small frames, 0.5 at 4K, where 8 of 24 searches then end on another
/// quantizer -- and the published SSIMULACRA2 code is the recursion; with the scorer at 0.3 % of a
/// pass either way, the search follows the published arithmetic.  A maintainer who can run fssimu2
/// settles it in minutes: tests/golden/pin_kit holds pairs on which the three modes are 0.1 to 3.8
/// points apart with the score of each -- and of 19 single-stage variants of the published algorithm --,
/// scripts/pin_blur_mode.py takes fssimu2's scores of the same files and names the mode that matches
/// within +-0.01, or the stage that differs (INTEGRATION.md 2e).  Set before the first call.
pub const Blur = enum(c_int) { fir = 0, recursive = 1, recursive_fma = 2 };
pub var blur: Blur = .recursive;

var g_ctx: ?*Ctx = null;
var g_ref_ptr: ?[*]const u8 = null;
var g_ref_len: usize = 0;
var g_ref_w: u32 = 0;
var g_ref_h: u32 = 0;
var g_ref_fp: u64 = 0;

fn check(rc: c_int) Error!void {
    return switch (rc) {
        0 => {},
        -1 => Error.InvalidArgument,
        -2 => Error.UnsupportedChannels,
        -3 => Error.OutOfMemory,
        -4 => Error.HipFailure,
        -5 => Error.NoReference,
        -6 => Error.NoDevice,
        else => Error.Unknown,
    };
}

fn context() Error!*Ctx {
    if (g_ctx) |c| return c;
    var c: ?*Ctx = null;
    try check(ssimu2_ctx_create(device, null, &c));
    if (blur != .fir) {
        const rc = ssimu2_ctx_set_blur(c, @intFromEnum(blur));
        if (rc != 0) {
            ssimu2_ctx_destroy(c);
            try check(rc);
        }
    }
    g_ctx = c;
    return c.?;
}

/// A cheap content fingerprint of the reference: FNV-1a over 4 KiB of it -- 64 runs of 64
/// consecutive bytes at evenly spaced positions (flat borders or letterbox bars defeat single
/// sampled bytes; a run that crosses 21 pixels mostly does not).  The cached reference is keyed on
/// (pointer, length, size, fingerprint): an allocator that hands a freed `e.rgb` address to the
/// next same-sized image no longer makes the shim score against the previous image's cached
/// planes (oavif today handles one image per process, so this cannot happen yet; a multi-image
/// host should still call invalidateReference()).
fn fingerprint(buf: []const u8) u64 {
    var h: u64 = 0xcbf29ce484222325;
    if (buf.len == 0) return h;
    const runs: usize = 64;
    const run_len: usize = @min(64, buf.len);
    const step: usize = @max((buf.len - run_len) / runs, 1);
    var start: usize = 0;
    var k: usize = 0;
    while (k < runs and start + run_len <= buf.len) : (k += 1) {
        for (buf[start .. start + run_len]) |b| {
            h = (h ^ b) *% 0x100000001b3;
        }
        start += step;
    }
    return h;
}

fn sameReference(reference: []const u8, width: u32, height: u32) bool {
    return g_ref_ptr != null and g_ref_ptr.? == reference.ptr and g_ref_len == reference.len and
        g_ref_w == width and g_ref_h == height and g_ref_fp == fingerprint(reference);
}

fn rememberReference(reference: []const u8, width: u32, height: u32) void {
    g_ref_ptr = reference.ptr;
    g_ref_len = reference.len;
    g_ref_w = width;
    g_ref_h = height;
    g_ref_fp = fingerprint(reference);
}

/// Explicit control for hosts that process several images in one process: upload `reference`
/// now (what computeSsimu2 would do on first sight of it) ...
pub fn setReference(reference: []const u8, width: u32, height: u32) Error!void {
    const ctx = try context();
    try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
    rememberReference(reference, width, height);
}

/// ... and forget it (call when `e.rgb` is freed or rewritten in place).
pub fn invalidateReference() void {
    g_ref_ptr = null;
}

/// Optional, for one-image runs: start the once-per-process GPU initialisation (0.15-0.35 s) on
/// a background thread; call it first thing in main() and the cost hides behind io.loadImage and
/// the first encode (INTEGRATION.md section 2d).
pub fn prefetch() void {
    _ = ssimu2_prefetch(device);
}

/// Wait for a prefetch still in flight.  Call before an early exit that never reached the scorer
/// (bad arguments, unreadable input), so HIP start-up does not race process teardown.
pub fn prefetchJoin() void {
    _ = ssimu2_prefetch_join(device);
}

/// Optional (INTEGRATION.md section 2b): a page-locked buffer for libavif to decode into -- point
/// `rgb.pixels` at it instead of calling avifRGBImageAllocatePixels (io.zig:475) and the upload of a pass
/// skips the HIP runtime's staging copy.  Measured a convenience, not a speed-up (the pageable path copies
/// at PCIe speed already).  Free with freeFrame before deinit().
pub fn allocFrame(bytes: usize) Error![]u8 {
    const ctx = try context();
    var p: ?*anyopaque = null;
    try check(ssimu2_host_alloc(ctx, bytes, &p));
    return @as([*]u8, @ptrCast(p.?))[0..bytes];
}

pub fn freeFrame(frame: []u8) void {
    if (g_ctx) |c| _ = ssimu2_host_free(c, frame.ptr);
}

/// Release the GPU context (optional; the process exit does it too).
pub fn deinit() void {
    if (g_ctx) |c| ssimu2_ctx_destroy(c);
    g_ctx = null;
    g_ref_ptr = null;
}

/// Same call shape as fssimu2 0.1.1 as seen from tq.zig:37.  `allocator` is unused (device
/// scratch lives in the context).  `error_map` is resolved at compile time: `null` (what oavif
/// passes) scores only; a `[]f32` of at least width * height elements also receives this library's
/// per-pixel error map (include/ssimu2_hip.h, DESIGN.md section 9 -- fssimu2's own map format is
/// unknown); any other type is a compile error.
pub fn computeSsimu2(
    allocator: std.mem.Allocator,
    reference: []const u8,
    distorted: []const u8,
    width: u32,
    height: u32,
    comptime channels: u32,
    error_map: anytype,
) Error!f64 {
    _ = allocator;
    const Map = @TypeOf(error_map);
    if (Map != @TypeOf(null) and Map != []f32)
        @compileError("computeSsimu2: error_map must be null or a []f32 of at least width * height elements, not " ++ @typeName(Map));
    const need: usize = @as(usize, width) * @as(usize, height) * channels;
    if (reference.len < need or distorted.len < need) return Error.InvalidArgument;
    if (Map == []f32) return scoreWithMap(reference, distorted, width, height, channels, error_map);
    const ctx = try context();
    var score: f64 = 0;
    if (cache_reference and channels == 3) {
        if (!sameReference(reference, width, height)) {
            try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
            rememberReference(reference, width, height);
        }
        const rc = ssimu2_score_against_reference(ctx, distorted.ptr, &score);
        if (rc == -5) { // the context lost its reference (e.g. a pair score in between): upload once more
            try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
            rememberReference(reference, width, height);
            try check(ssimu2_score_against_reference(ctx, distorted.ptr, &score));
            return score;
        }
        try check(rc);
        return score;
    }
    // ssimu2_score_rgb8 overwrites the context's reference planes: the shim's record of a cached
    // reference must not outlive them
    g_ref_ptr = null;
    try check(ssimu2_score_rgb8(ctx, reference.ptr, distorted.ptr, width, height, channels, &score));
    return score;
}

// computeSsimu2 with an error map: the same reference caching, through the map entry points
// (whose score is bit-identical to the plain calls').
fn scoreWithMap(reference: []const u8, distorted: []const u8, width: u32, height: u32, channels: u32, map: []f32) Error!f64 {
    if (map.len < @as(usize, width) * @as(usize, height)) return Error.InvalidArgument;
    const ctx = try context();
    var score: f64 = 0;
    if (cache_reference and channels == 3) {
        if (!sameReference(reference, width, height)) {
            try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
            rememberReference(reference, width, height);
        }
        const rc = ssimu2_error_map_against_reference(ctx, distorted.ptr, map.ptr, &score);
        if (rc == -5) { // the context lost its reference: upload once more
            try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
            rememberReference(reference, width, height);
            try check(ssimu2_error_map_against_reference(ctx, distorted.ptr, map.ptr, &score));
            return score;
        }
        try check(rc);
        return score;
    }
    g_ref_ptr = null;
    try check(ssimu2_error_map_rgb8(ctx, reference.ptr, distorted.ptr, width, height, channels, map.ptr, &score));
    return score;
}

/// Optional deeper hand-off (needs a small edit of oavif, INTEGRATION.md section 2b): score
/// libavif's decoded `avifRGBImage` as it is -- `pixels` = rgb.pixels, `row_bytes` = rgb.rowBytes,
/// `src_channels` = 3 or 4 -- against `reference`, so that the per-pixel copy loop of
/// io.decodeAvifToRgb (io.zig:654-663) and its w*h*3 allocation (io.zig:649) disappear from
/// every pass; alpha bytes and row padding are dropped on the device.  Same score, bit for bit,
/// as computeSsimu2 on the copied frame.
pub fn computeSsimu2Decoded(
    reference: []const u8,
    pixels: [*]const u8,
    row_bytes: u32,
    src_channels: u32,
    width: u32,
    height: u32,
) Error!f64 {
    const need: usize = @as(usize, width) * @as(usize, height) * 3;
    if (reference.len < need) return Error.InvalidArgument;
    const ctx = try context();
    if (!cache_reference or !sameReference(reference, width, height)) {
        try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
        rememberReference(reference, width, height);
    }
    var score: f64 = 0;
    try check(ssimu2_score_against_reference_strided(ctx, pixels, row_bytes, src_channels, &score));
    return score;
}

/// High-bit-depth pair score (include/ssimu2_hip.h, DESIGN.md section 10): `reference` and `distorted` are
/// interleaved RGB u16 samples of `bit_depth` bits (8..16), as libavif's avifRGBImage holds them at depth > 8 and as
/// a 16-bit PNG decodes.  Scored at full precision; a 16-bit frame of 257 * u gives the 8-bit score of u bit for bit.
/// Not reference-cached (a pair call replaces the context's cached reference, so the next cached call re-uploads).
pub fn computeSsimu2Hbd(
    reference: []const u16,
    distorted: []const u16,
    width: u32,
    height: u32,
    bit_depth: u32,
) Error!f64 {
    const need: usize = @as(usize, width) * @as(usize, height) * 3;
    if (reference.len < need or distorted.len < need) return Error.InvalidArgument;
    const ctx = try context();
    invalidateReference();
    var score: f64 = 0;
    try check(ssimu2_score_rgb16(ctx, reference.ptr, distorted.ptr, width, height, 3, bit_depth, &score));
    return score;
}

/// The `--tenbit 1` hand-off (INTEGRATION.md section 2f): an 8-bit source `reference` against libavif's decode of a
/// probe at rgb.depth = 16 (`pixels` = rgb.pixels as u16, `row_bytes` = rgb.rowBytes, `src_channels` = 3 or 4,
/// `bit_depth` = rgb.depth), so that a 10-bit encode is judged at full precision instead of on an 8-bit rounding of
/// itself.  The reference is cached as in computeSsimu2Decoded; alpha and row padding are skipped on the device.
pub fn computeSsimu2DecodedHbd(
    reference: []const u8,
    pixels: [*]const u16,
    row_bytes: u32,
    src_channels: u32,
    bit_depth: u32,
    width: u32,
    height: u32,
) Error!f64 {
    const need: usize = @as(usize, width) * @as(usize, height) * 3;
    if (reference.len < need) return Error.InvalidArgument;
    const ctx = try context();
    if (!cache_reference or !sameReference(reference, width, height)) {
        try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
        rememberReference(reference, width, height);
    }
    var score: f64 = 0;
    try check(ssimu2_score_against_reference_strided16(ctx, pixels, row_bytes, src_channels, bit_depth, &score));
    return score;
}

var g_batch_ctx: ?*Ctx = null;

// Batches run in the FIR mode only (include/ssimu2_hip.h "Batch scoring"), whatever `blur` the search path uses:
// they get a context of their own, which a bare ssimu2_ctx_create leaves in SSIMU2_BLUR_FIR.
fn batchContext() Error!*Ctx {
    if (g_batch_ctx) |c| return c;
    var c: ?*Ctx = null;
    try check(ssimu2_ctx_create(device, null, &c));
    g_batch_ctx = c;
    return c.?;
}

/// Release the batch context (optional, as deinit()).
pub fn deinitBatch() void {
    if (g_batch_ctx) |c| ssimu2_ctx_destroy(c);
    g_batch_ctx = null;
}

/// Score `references.len` pairs of ONE size in one launch set (ssimu2_score_batch_rgb8): a corpus of thumbnails, tiles
/// or video frames, where a single small score cannot fill the GPU.  `scores` receives one score per pair in input
/// order, each independent of the batch it travelled in.  8-bit RGB, SSIMU2_BLUR_FIR; at most 4096 pairs per call
/// (SSIMU2_MAX_BATCH).  `allocator` holds the two pointer arrays for the duration of the call.
pub fn computeSsimu2Batch(
    allocator: std.mem.Allocator,
    references: []const []const u8,
    distorted: []const []const u8,
    width: u32,
    height: u32,
    scores: []f64,
) Error!void {
    const n = references.len;
    if (distorted.len != n or scores.len < n or n > 4096) return Error.InvalidArgument;
    if (n == 0) return;
    const need: usize = @as(usize, width) * @as(usize, height) * 3;
    const refs = allocator.alloc([*]const u8, n) catch return Error.OutOfMemory;
    defer allocator.free(refs);
    const dists = allocator.alloc([*]const u8, n) catch return Error.OutOfMemory;
    defer allocator.free(dists);
    for (references, distorted, 0..) |r, d, i| {
        if (r.len < need or d.len < need) return Error.InvalidArgument;
        refs[i] = r.ptr;
        dists[i] = d.ptr;
    }
    const ctx = try batchContext();
    try check(ssimu2_score_batch_rgb8(ctx, refs.ptr, dists.ptr, @intCast(n), width, height, scores.ptr));
}

/// Several probes of one image in one launch set (ssimu2_score_batch_against_reference): `reference` is uploaded and
/// cached on the batch context as computeSsimu2 caches it, every frame of `distorted` is scored against it.
pub fn computeSsimu2BatchAgainst(
    allocator: std.mem.Allocator,
    reference: []const u8,
    distorted: []const []const u8,
    width: u32,
    height: u32,
    scores: []f64,
) Error!void {
    const n = distorted.len;
    const need: usize = @as(usize, width) * @as(usize, height) * 3;
    if (reference.len < need or scores.len < n or n > 4096) return Error.InvalidArgument;
    if (n == 0) return;
    const dists = allocator.alloc([*]const u8, n) catch return Error.OutOfMemory;
    defer allocator.free(dists);
    for (distorted, 0..) |d, i| {
        if (d.len < need) return Error.InvalidArgument;
        dists[i] = d.ptr;
    }
    const ctx = try batchContext();
    try check(ssimu2_set_reference(ctx, reference.ptr, width, height));
    try check(ssimu2_score_batch_against_reference(ctx, dists.ptr, @intCast(n), scores.ptr));
}
