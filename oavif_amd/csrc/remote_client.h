// Client side of the resident scoring service, and the wire protocol both sides speak.
//
// With OAVIF_SCORER_SOCKET set, ssimu2_ctx_create (ssimu2_hip.hip) makes a REMOTE context: a connection to an
// oavif_scored process (oavif_scored.cpp) that owns the GPU.  Every entry point of include/ssimu2_hip.h then starts
// with a dispatch into the functions below, and the process makes no HIP call for that context.  This translation
// unit is HIP-free (no hip/* include): it also compiles with plain g++ for the CPU tests.
//
// Protocol (version kProto; same machine, same byte order, so plain structs): after connect() the client sends Hello
// (with the context's memfd as SCM_RIGHTS when it wants a context) and reads HelloReply; then any number of Request ->
// Reply pairs, each a fixed-size struct.  Frames, maps, score arrays and averages never cross the socket: a Request
// names byte ranges of the shared memory file, which the server maps once and remaps when the file has grown.
#ifndef OAVIF_REMOTE_CLIENT_H_
#define OAVIF_REMOTE_CLIENT_H_

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/ssimu2_hip.h"

namespace ssimu2r {

// ---- wire ----------------------------------------------------------------------------------------
constexpr uint32_t kMagic = 0x53324356u;  // "VC2S"
constexpr uint32_t kProto = 1;
constexpr uint64_t kNull = ~0ull;         // a null pointer of the caller, as a range offset
constexpr uint32_t kTextMax = 512;
constexpr uint64_t kMaxPixels = (1ull << 31) / 3;  // the library's own frame limit (check_args)
constexpr uint64_t kShmMax = 1ull << 40;

enum : uint32_t { kHelloWantCtx = 1 };
struct Hello {
    uint32_t magic, proto, flags, pad;
    uint64_t shm_size;  // size of the memfd passed along (kHelloWantCtx)
    char version[kTextMax];  // the client's ssimu2_version(), NUL-terminated
};
struct HelloReply {
    uint32_t magic;
    int32_t rc;  // SSIMU2_OK, or why there is no context (SSIMU2_ERR_OOM: every slot taken; NO_DEVICE: refused)
    ssimu2_device_info info;  // the server's device
    char text[kTextMax];
};

enum Op : uint32_t {
    kOpSetBlur = 1,        // a0 mode
    kOpScoreRgb8,          // a0 w, a1 h, a2 channels; in0 ref, in1 dist
    kOpSetRef,             // a0 w, a1 h; in0
    kOpScoreRef,           // in0
    kOpScoreStrided,       // a0 row_bytes, a1 channels; in0
    kOpScoreRgb16,         // a0 w, a1 h, a2 channels, a3 bit_depth; in0, in1
    kOpSetRef16,           // a0 w, a1 h, a2 bit_depth; in0
    kOpScoreRef16,         // a0 bit_depth; in0
    kOpScoreStrided16,     // a0 row_bytes, a1 channels, a2 bit_depth; in0
    kOpMapRgb8,            // as kOpScoreRgb8; out: w * h floats
    kOpMapRef,             // in0; out: ref_w * ref_h floats
    kOpLastAverages,       // out: 108 doubles; Reply::i0 = scales
    kOpBatchRgb8,          // a0 n, a1 w, a2 h; in0 / in1: n uint64 offsets of the items (kNull = null item); out: n doubles
    kOpBatchRef,           // a0 n; in0: n uint64 offsets; out: n doubles
    kOpLastBatchAverages,  // a0 item; out: 108 doubles; Reply::i0 = scales
    kOpCount
};
enum : uint32_t { kNoScore = 1, kNoOut = 2 };  // Request::flags: the caller's out_score / out array is null
struct Range { uint64_t off, len; };           // off == kNull: the caller's pointer is null
struct Request {
    uint32_t magic, op;
    uint32_t a[4];
    uint32_t flags, pad;
    uint64_t shm_size;  // the file's size now: the server remaps when it exceeds its mapping
    Range in[2], out;
};
struct Reply {
    uint32_t magic;
    int32_t rc;
    double score;
    int32_t i0;
    uint32_t pad;
    char text[kTextMax];  // ssimu2_last_error of the server's context after the call
};

// What both ends know of the server context's reference without asking it: set by a successful set_reference, dropped
// by a successful pair score or blur switch.  `have` may stay true where the library has dropped the reference after a
// failed call (the library then answers SSIMU2_ERR_NO_REFERENCE itself); it is never false while the library holds one,
// so the bytes a call reads are always there.
struct RefMirror {
    bool have = false;
    uint32_t w = 0, h = 0;
    void update(const Request& q, int rc) {
        if (rc != SSIMU2_OK) return;
        switch (q.op) {
            case kOpSetRef: case kOpSetRef16: have = true; w = q.a[0]; h = q.a[1]; break;
            case kOpSetBlur: case kOpScoreRgb8: case kOpScoreRgb16: case kOpMapRgb8: have = false; break;
            default: break;
        }
    }
};

// Bytes the library reads behind each input pointer and writes behind the output array of request `q`, when it gets
// that far; 0 where it refuses the call before it touches the pointer.  The client stages exactly these, the server
// checks every range against them before it calls anything.
struct Needs { uint64_t in[2], out; };
inline Needs needs(const Request& q, const RefMirror& m) {
    Needs n = {{0, 0}, 0};
    const uint64_t a0 = q.a[0], a1 = q.a[1];
    const uint64_t refpx = m.have ? (uint64_t)m.w * m.h : 0;
    auto frame = [](uint64_t w, uint64_t h) { return w && h && w * h <= kMaxPixels ? w * h : 0; };
    auto strided = [&](uint64_t row_bytes, uint64_t ch, uint64_t sample) -> uint64_t {
        if (!refpx || (ch != 3 && ch != 4) || row_bytes < (uint64_t)m.w * ch * sample) return 0;
        return row_bytes * (m.h - 1) + (uint64_t)m.w * ch * sample;
    };
    switch (q.op) {
        case kOpScoreRgb8: n.in[0] = n.in[1] = frame(a0, a1) * 3; break;
        case kOpMapRgb8: n.in[0] = n.in[1] = frame(a0, a1) * 3; n.out = frame(a0, a1) * 4; break;
        case kOpSetRef: n.in[0] = frame(a0, a1) * 3; break;
        case kOpScoreRef: n.in[0] = refpx * 3; break;
        case kOpMapRef: n.in[0] = refpx * 3; n.out = refpx * 4; break;
        case kOpScoreStrided: n.in[0] = strided(a0, a1, 1); break;
        case kOpScoreRgb16: n.in[0] = n.in[1] = frame(a0, a1) * 6; break;
        case kOpSetRef16: n.in[0] = frame(a0, a1) * 6; break;
        case kOpScoreRef16: n.in[0] = refpx * 6; break;
        case kOpScoreStrided16: n.in[0] = strided(a0, a1, 2); break;
        case kOpLastAverages: case kOpLastBatchAverages: n.out = 108 * sizeof(double); break;
        case kOpBatchRgb8:
            if (a0 && a0 <= SSIMU2_MAX_BATCH) { n.in[0] = n.in[1] = a0 * 8; n.out = a0 * 8; }
            break;
        case kOpBatchRef:
            if (a0 && a0 <= SSIMU2_MAX_BATCH) { n.in[0] = a0 * 8; n.out = a0 * 8; }
            break;
        default: break;
    }
    return n;
}
// Bytes of one item of a batch request (behind every offset of its offset arrays).
inline uint64_t batch_item_bytes(const Request& q, const RefMirror& m) {
    if (q.op == kOpBatchRgb8) {
        const uint64_t w = q.a[1], h = q.a[2];
        return w && h && w * h <= kMaxPixels ? w * h * 3 : 0;
    }
    return m.have ? (uint64_t)m.w * m.h * 3 : 0;
}

// ---- client --------------------------------------------------------------------------------------
struct Remote;

// The value of OAVIF_SCORER_SOCKET with %d replaced by `device`; empty when the variable is unset or empty.
std::string socket_path(int device);
inline bool enabled() {
    const char* s = getenv("OAVIF_SCORER_SOCKET");
    return s && *s;
}

// Connect and shake hands.  `err` receives the text for ssimu2_last_error(NULL).
int create(int device, void* hip_stream, const char* version, Remote** out, ssimu2_device_info* info, std::string* err);
int query_device(int device, const char* version, ssimu2_device_info* out, std::string* err);
void destroy(Remote* r);
const char* last_error(const Remote* r);
int unsupported(Remote* r, const char* what);  // the *_device forms, ssimu2_enqueue_*, ssimu2_wait, the instrumented hooks

int host_alloc(Remote* r, size_t bytes, void** out_ptr);
int host_free(Remote* r, void* ptr);
int set_blur(Remote* r, int mode);
int score_rgb8(Remote* r, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h, uint32_t channels, double* out);
int set_reference(Remote* r, const uint8_t* ref, uint32_t w, uint32_t h);
int score_against_reference(Remote* r, const uint8_t* dist, double* out);
int score_strided(Remote* r, const uint8_t* px, uint32_t row_bytes, uint32_t channels, double* out);
int score_rgb16(Remote* r, const uint16_t* ref, const uint16_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                uint32_t bit_depth, double* out);
int set_reference_rgb16(Remote* r, const uint16_t* ref, uint32_t w, uint32_t h, uint32_t bit_depth);
int score_against_reference_rgb16(Remote* r, const uint16_t* dist, uint32_t bit_depth, double* out);
int score_strided16(Remote* r, const uint16_t* px, uint32_t row_bytes, uint32_t channels, uint32_t bit_depth, double* out);
int error_map_rgb8(Remote* r, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                   float* out_map, double* out);
int error_map_against_reference(Remote* r, const uint8_t* dist, float* out_map, double* out);
int last_averages(Remote* r, double* out, int* out_num_scales);
int score_batch_rgb8(Remote* r, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n, uint32_t w,
                     uint32_t h, double* out_scores);
int score_batch_against_reference(Remote* r, const uint8_t* const* dists, uint32_t n, double* out_scores);
int last_batch_averages(Remote* r, uint32_t item, double* out, int* out_num_scales);

}  // namespace ssimu2r

#endif  // OAVIF_REMOTE_CLIENT_H_
