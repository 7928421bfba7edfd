// Client side of the resident scoring service: see remote_client.h and DESIGN.md section 12.  No HIP here.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE 1
#endif
#include "remote_client.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <sys/socket.h>
#include <sys/time.h>
#include <sys/un.h>
#include <unistd.h>

#include <new>
#include <vector>

namespace ssimu2r {

namespace {

constexpr uint64_t kPage = 4096;
inline uint64_t page_up(uint64_t v) { return (v + kPage - 1) & ~(kPage - 1); }

struct Block {  // one mapping of a page-aligned range of the context's file
    uint8_t* base = nullptr;
    uint64_t len = 0, off = 0;
};

double timeout_seconds() {
    const char* s = getenv("OAVIF_SCORER_TIMEOUT_S");
    double t = s && *s ? atof(s) : 0.0;
    return t > 0.0 ? t : 120.0;
}

}  // namespace

struct Remote {
    int sock = -1, memfd = -1;
    uint64_t file_size = 0;  // bytes of the file handed out so far (its size)
    std::vector<Range> free_ranges;
    std::vector<Block> blocks;  // ssimu2_host_alloc
    Block stage;                // frames from any other pointer, and everything that comes back
    RefMirror ref;
    bool dead = false;  // connection lost or timed out: every later call returns the same error
    std::string err, path;

    int fail(int code, const std::string& what) {
        err = what;
        return code;
    }
    int lost(bool timed_out) {
        dead = true;
        if (sock >= 0) close(sock);
        sock = -1;
        return fail(SSIMU2_ERR_HIP, timed_out ? "scoring service: connection timed out" : "scoring service: connection lost");
    }
};

namespace {

// 1 = done, 0 = peer gone / error, -1 = timed out
int send_all(int fd, const void* p, size_t n) {
    const char* b = (const char*)p;
    while (n) {
        const ssize_t k = send(fd, b, n, MSG_NOSIGNAL);
        if (k < 0 && errno == EINTR) continue;
        if (k < 0) return errno == EAGAIN || errno == EWOULDBLOCK ? -1 : 0;
        b += k;
        n -= (size_t)k;
    }
    return 1;
}
int recv_all(int fd, void* p, size_t n) {
    char* b = (char*)p;
    while (n) {
        const ssize_t k = recv(fd, b, n, 0);
        if (k < 0 && errno == EINTR) continue;
        if (k < 0) return errno == EAGAIN || errno == EWOULDBLOCK ? -1 : 0;
        if (k == 0) return 0;
        b += k;
        n -= (size_t)k;
    }
    return 1;
}

// Hello with the file descriptor riding along.
int send_hello(int fd, const Hello& h, int pass_fd) {
    struct iovec iov = {(void*)&h, sizeof h};
    struct msghdr m;
    memset(&m, 0, sizeof m);
    m.msg_iov = &iov;
    m.msg_iovlen = 1;
    alignas(struct cmsghdr) char ctl[CMSG_SPACE(sizeof(int))];
    if (pass_fd >= 0) {
        memset(ctl, 0, sizeof ctl);
        m.msg_control = ctl;
        m.msg_controllen = sizeof ctl;
        struct cmsghdr* c = CMSG_FIRSTHDR(&m);
        c->cmsg_level = SOL_SOCKET;
        c->cmsg_type = SCM_RIGHTS;
        c->cmsg_len = CMSG_LEN(sizeof(int));
        memcpy(CMSG_DATA(c), &pass_fd, sizeof(int));
    }
    for (;;) {
        const ssize_t k = sendmsg(fd, &m, MSG_NOSIGNAL);
        if (k < 0 && errno == EINTR) continue;
        if (k < 0) return errno == EAGAIN || errno == EWOULDBLOCK ? -1 : 0;
        if ((size_t)k == sizeof h) return 1;
        return send_all(fd, (const char*)&h + k, sizeof h - (size_t)k);  // the descriptor went with the first byte
    }
}

// Connect and shake hands; returns the socket or -1 with *rc / *err set.
int dial(int device, const char* version, int pass_fd, uint64_t shm_size, HelloReply* rep, int* rc, std::string* err,
         std::string* path_out) {
    const std::string path = socket_path(device);
    if (path_out) *path_out = path;
    auto refuse = [&](int code, const std::string& why) {
        *rc = code;
        *err = "scoring service at " + path + ": " + why;
        return -1;
    };
    struct sockaddr_un sa;
    memset(&sa, 0, sizeof sa);
    sa.sun_family = AF_UNIX;
    if (path.size() >= sizeof sa.sun_path) return refuse(SSIMU2_ERR_NO_DEVICE, "socket path too long");
    memcpy(sa.sun_path, path.c_str(), path.size());
    const int fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (fd < 0) return refuse(SSIMU2_ERR_NO_DEVICE, std::string("socket: ") + strerror(errno));
    const double t = timeout_seconds();
    struct timeval tv;
    tv.tv_sec = (time_t)t;
    tv.tv_usec = (suseconds_t)((t - (double)tv.tv_sec) * 1e6);
    (void)setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    (void)setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof tv);
    if (connect(fd, (struct sockaddr*)&sa, sizeof sa) != 0) {
        const int e = errno;
        close(fd);
        return refuse(SSIMU2_ERR_NO_DEVICE, std::string("cannot connect (") + strerror(e) + "); OAVIF_SCORER_SOCKET is set, "
                                            "so no local GPU is tried");
    }
    Hello h;
    memset(&h, 0, sizeof h);
    h.magic = kMagic;
    h.proto = kProto;
    h.flags = pass_fd >= 0 ? (uint32_t)kHelloWantCtx : 0u;
    h.shm_size = shm_size;
    snprintf(h.version, sizeof h.version, "%s", version);
    if (send_hello(fd, h, pass_fd) != 1 || recv_all(fd, rep, sizeof *rep) != 1) {
        close(fd);
        return refuse(SSIMU2_ERR_NO_DEVICE, "handshake not answered (protocol version refused, or not a scoring service)");
    }
    rep->text[kTextMax - 1] = 0;
    if (rep->magic != kMagic) {
        close(fd);
        return refuse(SSIMU2_ERR_NO_DEVICE, "handshake answered by something else");
    }
    if (rep->rc != SSIMU2_OK) {
        close(fd);
        return refuse(rep->rc, rep->text);
    }
    return fd;
}

// A page-aligned range of the file, mapped.
bool map_range(Remote* r, uint64_t bytes, Block* b) {
    const uint64_t len = page_up(bytes);
    uint64_t off = kNull;
    for (size_t i = 0; i < r->free_ranges.size(); ++i)
        if (r->free_ranges[i].len >= len) {
            off = r->free_ranges[i].off;
            r->free_ranges[i].off += len;
            r->free_ranges[i].len -= len;
            if (!r->free_ranges[i].len) r->free_ranges.erase(r->free_ranges.begin() + (long)i);
            break;
        }
    const bool grown = off == kNull;
    if (grown) {
        if (r->file_size + len > kShmMax || ftruncate(r->memfd, (off_t)(r->file_size + len)) != 0) return false;
        off = r->file_size;
        r->file_size += len;
    }
    void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_SHARED, r->memfd, (off_t)off);
    if (p == MAP_FAILED) {
        r->free_ranges.push_back(Range{off, len});
        return false;
    }
    b->base = (uint8_t*)p;
    b->len = len;
    b->off = off;
    return true;
}
void unmap_range(Remote* r, Block* b) {
    if (!b->base) return;
    munmap(b->base, b->len);
    (void)fallocate(r->memfd, FALLOC_FL_PUNCH_HOLE | FALLOC_FL_KEEP_SIZE, (off_t)b->off, (off_t)b->len);  // give the pages back
    r->free_ranges.push_back(Range{b->off, b->len});
    *b = Block();
}

// One call: where each input lies in the file (copied into the staging range unless it already lies in a block of
// ssimu2_host_alloc), room for the output, the round trip, the output copied out.
struct Call {
    Remote* r;
    Request q;
    uint64_t cursor = 0;
    Call(Remote* r_, uint32_t op, uint32_t a0 = 0, uint32_t a1 = 0, uint32_t a2 = 0, uint32_t a3 = 0) : r(r_) {
        memset(&q, 0, sizeof q);
        q.magic = kMagic;
        q.op = op;
        q.a[0] = a0; q.a[1] = a1; q.a[2] = a2; q.a[3] = a3;
        q.in[0].off = q.in[1].off = q.out.off = kNull;
    }
    bool in_block(const void* p, uint64_t len, uint64_t* off) const {
        const uint8_t* b = (const uint8_t*)p;
        for (const Block& k : r->blocks)
            if (b >= k.base && b + len <= k.base + k.len) {
                *off = k.off + (uint64_t)(b - k.base);
                return true;
            }
        return false;
    }
    // bytes of staging an input of `len` at `p` takes (0 when it lies in shared memory already)
    uint64_t stage_bytes(const void* p, uint64_t len) const {
        uint64_t off;
        return !p || in_block(p, len, &off) ? 0 : ((len + 64 + 63) & ~63ull);
    }
    bool reserve(uint64_t bytes) {
        cursor = 0;
        if (bytes <= r->stage.len) return true;
        unmap_range(r, &r->stage);
        return map_range(r, bytes + bytes / 4, &r->stage);
    }
    // The file offset of `len` bytes at `p`: in place, or copied.  The offset keeps the pointer's parity, so that the
    // library on the other side sees an odd address where the caller passed one.
    uint64_t place(const void* p, uint64_t len) {
        if (!p) return kNull;
        uint64_t off;
        if (in_block(p, len, &off)) return off;
        const uint64_t at = cursor + ((uintptr_t)p & 1u);
        if (len) memcpy(r->stage.base + at, p, len);
        cursor += (len + 64 + 63) & ~63ull;
        return r->stage.off + at;
    }
    uint64_t place_out(uint64_t len) {
        const uint64_t at = cursor;
        cursor += (len + 63) & ~63ull;
        return r->stage.off + at;
    }
    const uint8_t* out_ptr() const { return r->stage.base + (q.out.off - r->stage.off); }

    int roundtrip(double* out_score, int* i0) {
        q.shm_size = r->file_size;
        int k = send_all(r->sock, &q, sizeof q);
        Reply rep;
        if (k == 1) k = recv_all(r->sock, &rep, sizeof rep);
        if (k != 1 || rep.magic != kMagic) return r->lost(k < 0);
        rep.text[kTextMax - 1] = 0;
        r->err = rep.text;
        r->ref.update(q, rep.rc);
        if (rep.rc == SSIMU2_OK) {
            if (out_score) *out_score = rep.score;
            if (i0) *i0 = rep.i0;
        }
        return rep.rc;
    }
};

// The shape of every single-frame call: up to two inputs, an optional output array, a score.
int simple(Remote* r, Call& c, const void* in0, const void* in1, void* out_arr, bool has_out, double* out_score,
           bool has_score, int* i0 = nullptr) {
    if (r->dead) return SSIMU2_ERR_HIP;
    const Needs n = needs(c.q, r->ref);
    if (!c.reserve(c.stage_bytes(in0, n.in[0]) + c.stage_bytes(in1, n.in[1]) + ((n.out + 63) & ~63ull)))
        return r->fail(SSIMU2_ERR_OOM, "scoring service: cannot grow the shared frame memory");
    c.q.in[0] = Range{c.place(in0, n.in[0]), n.in[0]};
    c.q.in[1] = Range{c.place(in1, n.in[1]), n.in[1]};
    if (has_out && out_arr) c.q.out = Range{c.place_out(n.out), n.out};
    if (has_out && !out_arr) c.q.flags |= kNoOut;
    if (has_score && !out_score) c.q.flags |= kNoScore;
    const int rc = c.roundtrip(out_score, i0);
    if (rc == SSIMU2_OK && has_out && out_arr && n.out) memcpy(out_arr, c.out_ptr(), n.out);
    return rc;
}

int batch(Remote* r, Call& c, const uint8_t* const* refs, bool has_refs, const uint8_t* const* dists, uint32_t n_items,
          double* out_scores) {
    if (r->dead) return SSIMU2_ERR_HIP;
    const Needs n = needs(c.q, r->ref);
    const uint64_t item = batch_item_bytes(c.q, r->ref);
    const uint8_t* const* arr[2] = {has_refs ? refs : dists, has_refs ? dists : nullptr};
    const uint32_t count = n.in[0] ? n_items : 0;  // 0: the library refuses the call before it reads an array
    uint64_t total = (n.out + 63) & ~63ull;
    for (int k = 0; k < 2; ++k) {
        if (!arr[k] || !count) continue;
        total += (uint64_t)count * 8 + 128;
        for (uint32_t i = 0; i < count; ++i) total += c.stage_bytes(arr[k][i], item);
    }
    if (!c.reserve(total)) return r->fail(SSIMU2_ERR_OOM, "scoring service: cannot grow the shared frame memory");
    for (int k = 0; k < 2; ++k) {
        if (!arr[k]) continue;  // stays kNull: a null array (or, for the second, no such argument)
        c.q.in[k] = Range{0, 0};
        if (!count) continue;
        std::vector<uint64_t> offs(count);
        for (uint32_t i = 0; i < count; ++i) offs[i] = c.place(arr[k][i], item);
        c.q.in[k] = Range{c.place(offs.data(), (uint64_t)count * 8), (uint64_t)count * 8};
    }
    if (out_scores) c.q.out = Range{c.place_out(n.out), n.out};
    else c.q.flags |= kNoOut;
    const int rc = c.roundtrip(nullptr, nullptr);
    if (rc == SSIMU2_OK && out_scores && n.out) memcpy(out_scores, c.out_ptr(), n.out);
    return rc;
}

}  // namespace

std::string socket_path(int device) {
    const char* s = getenv("OAVIF_SCORER_SOCKET");
    std::string out;
    if (!s) return out;
    for (; *s; ++s) {
        if (s[0] == '%' && s[1] == 'd') {
            out += std::to_string(device);
            ++s;
        } else {
            out += *s;
        }
    }
    return out;
}

int create(int device, void* hip_stream, const char* version, Remote** out, ssimu2_device_info* info, std::string* err) {
    if (!out) return SSIMU2_ERR_INVALID_ARG;
    *out = nullptr;
    if (hip_stream) {
        *err = "scoring service: a caller's hip_stream means nothing to another process (OAVIF_SCORER_SOCKET is set)";
        return SSIMU2_ERR_INVALID_ARG;
    }
    Remote* r = new (std::nothrow) Remote();
    if (!r) return SSIMU2_ERR_OOM;
    r->memfd = memfd_create("oavif_scorer_frames", MFD_CLOEXEC | MFD_ALLOW_SEALING);
    if (r->memfd < 0 || fcntl(r->memfd, F_ADD_SEALS, F_SEAL_SHRINK) != 0) {  // the server maps it: it must never shrink
        *err = std::string("scoring service: memfd_create: ") + strerror(errno);
        destroy(r);
        return SSIMU2_ERR_OOM;
    }
    HelloReply rep;
    int rc = SSIMU2_ERR_NO_DEVICE;
    r->sock = dial(device, version, r->memfd, 0, &rep, &rc, err, &r->path);
    if (r->sock < 0) {
        destroy(r);
        return rc;
    }
    if (info) *info = rep.info;
    *out = r;
    return SSIMU2_OK;
}

int query_device(int device, const char* version, ssimu2_device_info* out, std::string* err) {
    HelloReply rep;
    int rc = SSIMU2_ERR_NO_DEVICE;
    const int fd = dial(device, version, -1, 0, &rep, &rc, err, nullptr);
    if (fd < 0) return rc;
    close(fd);
    *out = rep.info;
    return SSIMU2_OK;
}

void destroy(Remote* r) {
    if (!r) return;
    if (r->sock >= 0) close(r->sock);  // the server returns the context to its pool
    for (Block& b : r->blocks) munmap(b.base, b.len);
    if (r->stage.base) munmap(r->stage.base, r->stage.len);
    if (r->memfd >= 0) close(r->memfd);
    delete r;
}

const char* last_error(const Remote* r) { return r->err.c_str(); }

int unsupported(Remote* r, const char* what) {
    if (r->dead) return SSIMU2_ERR_HIP;
    return r->fail(SSIMU2_ERR_UNSUPPORTED, std::string(what) + ": not served by the scoring service (a device pointer or "
                                           "an enqueued score of this process means nothing to it); unset OAVIF_SCORER_SOCKET");
}

int host_alloc(Remote* r, size_t bytes, void** out_ptr) {
    if (!out_ptr || bytes == 0) return r->fail(SSIMU2_ERR_INVALID_ARG, "ssimu2_host_alloc: null out_ptr or zero bytes");
    *out_ptr = nullptr;
    if (r->dead) return SSIMU2_ERR_HIP;
    Block b;
    if (!map_range(r, bytes, &b)) return r->fail(SSIMU2_ERR_OOM, "scoring service: cannot grow the shared frame memory");
    r->blocks.push_back(b);
    *out_ptr = b.base;
    return SSIMU2_OK;
}

int host_free(Remote* r, void* ptr) {
    if (!ptr) return SSIMU2_OK;
    for (size_t i = 0; i < r->blocks.size(); ++i)
        if (r->blocks[i].base == ptr) {
            unmap_range(r, &r->blocks[i]);
            r->blocks.erase(r->blocks.begin() + (long)i);
            return SSIMU2_OK;
        }
    return r->fail(SSIMU2_ERR_INVALID_ARG, "ssimu2_host_free: not a pointer of ssimu2_host_alloc on this context");
}

int set_blur(Remote* r, int mode) {
    Call c(r, kOpSetBlur, (uint32_t)mode);
    return simple(r, c, nullptr, nullptr, nullptr, false, nullptr, false);
}
int score_rgb8(Remote* r, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h, uint32_t channels, double* out) {
    Call c(r, kOpScoreRgb8, w, h, channels);
    return simple(r, c, ref, dist, nullptr, false, out, true);
}
int set_reference(Remote* r, const uint8_t* ref, uint32_t w, uint32_t h) {
    Call c(r, kOpSetRef, w, h);
    return simple(r, c, ref, nullptr, nullptr, false, nullptr, false);
}
int score_against_reference(Remote* r, const uint8_t* dist, double* out) {
    Call c(r, kOpScoreRef);
    return simple(r, c, dist, nullptr, nullptr, false, out, true);
}
int score_strided(Remote* r, const uint8_t* px, uint32_t row_bytes, uint32_t channels, double* out) {
    Call c(r, kOpScoreStrided, row_bytes, channels);
    return simple(r, c, px, nullptr, nullptr, false, out, true);
}
int score_rgb16(Remote* r, const uint16_t* ref, const uint16_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                uint32_t bit_depth, double* out) {
    Call c(r, kOpScoreRgb16, w, h, channels, bit_depth);
    return simple(r, c, ref, dist, nullptr, false, out, true);
}
int set_reference_rgb16(Remote* r, const uint16_t* ref, uint32_t w, uint32_t h, uint32_t bit_depth) {
    Call c(r, kOpSetRef16, w, h, bit_depth);
    return simple(r, c, ref, nullptr, nullptr, false, nullptr, false);
}
int score_against_reference_rgb16(Remote* r, const uint16_t* dist, uint32_t bit_depth, double* out) {
    Call c(r, kOpScoreRef16, bit_depth);
    return simple(r, c, dist, nullptr, nullptr, false, out, true);
}
int score_strided16(Remote* r, const uint16_t* px, uint32_t row_bytes, uint32_t channels, uint32_t bit_depth, double* out) {
    Call c(r, kOpScoreStrided16, row_bytes, channels, bit_depth);
    return simple(r, c, px, nullptr, nullptr, false, out, true);
}
int error_map_rgb8(Remote* r, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                   float* out_map, double* out) {
    Call c(r, kOpMapRgb8, w, h, channels);
    return simple(r, c, ref, dist, out_map, true, out, true);
}
int error_map_against_reference(Remote* r, const uint8_t* dist, float* out_map, double* out) {
    Call c(r, kOpMapRef);
    return simple(r, c, dist, nullptr, out_map, true, out, true);
}
int last_averages(Remote* r, double* out, int* out_num_scales) {
    Call c(r, kOpLastAverages);
    return simple(r, c, nullptr, nullptr, out, true, nullptr, false, out_num_scales);
}
int score_batch_rgb8(Remote* r, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n, uint32_t w,
                     uint32_t h, double* out_scores) {
    Call c(r, kOpBatchRgb8, n, w, h);
    return batch(r, c, refs, true, dists, n, out_scores);
}
int score_batch_against_reference(Remote* r, const uint8_t* const* dists, uint32_t n, double* out_scores) {
    Call c(r, kOpBatchRef, n);
    return batch(r, c, nullptr, false, dists, n, out_scores);
}
int last_batch_averages(Remote* r, uint32_t item, double* out, int* out_num_scales) {
    Call c(r, kOpLastBatchAverages, item);
    return simple(r, c, nullptr, nullptr, out, true, nullptr, false, out_num_scales);
}

}  // namespace ssimu2r
