// oavif_scored -- the resident scoring service.
//
// One process owns the GPU and serves the scorer of include/ssimu2_hip.h over a Unix-domain socket, so that any
// number of per-image processes (the reference's scripts/measure.py starts one `oavif` per image) cost one HIP
// start-up and hold the GPU open from one process.  Clients are ordinary users of the library with
// OAVIF_SCORER_SOCKET set (remote_client.cpp); this program is plain C++ over the public header and knows nothing
// of HIP.  One connection = one ssimu2_ctx on one thread; contexts of closed connections wait in a pool.
//
//   oavif_scored --socket PATH [--device D] [--max-contexts N=16] [--idle-exit SECONDS] [--max-lifetime SECONDS]
//                [--parent-pid PID]
#ifndef _GNU_SOURCE
#define _GNU_SOURCE 1
#endif
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <sys/un.h>
#include <time.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "remote_client.h"  // the wire structs and the byte counts both sides agree on

using namespace ssimu2r;

namespace {

struct Options {
    std::string socket;
    int device = 0;
    int max_contexts = 16;
    double idle_exit = 0, max_lifetime = 0;  // 0 = never
    long parent_pid = 0;
} g_opt;

volatile sig_atomic_t g_signal = 0;

std::mutex g_mu;  // everything below
std::condition_variable g_cv;
std::vector<ssimu2_ctx*> g_pool;  // idle contexts, reset
std::vector<int> g_conns;         // sockets of live connections (for shutdown)
int g_active = 0;                 // connections that hold a context
double g_idle_since = 0;          // when g_active last fell to 0
bool g_fault = false;             // a call returned SSIMU2_ERR_HIP: nothing more goes to the GPU
std::string g_fault_text;
double g_fault_at = 0;
ssimu2_device_info g_info;

double now() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

void on_signal(int s) { g_signal = s; }

bool send_all(int fd, const void* p, size_t n) {
    const char* b = (const char*)p;
    while (n) {
        const ssize_t k = send(fd, b, n, MSG_NOSIGNAL);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return false;
        b += k;
        n -= (size_t)k;
    }
    return true;
}
bool recv_all(int fd, void* p, size_t n) {
    char* b = (char*)p;
    while (n) {
        const ssize_t k = recv(fd, b, n, 0);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return false;
        b += k;
        n -= (size_t)k;
    }
    return true;
}

// The Hello and the descriptor that rides on it (-1 when there is none).
bool recv_hello(int fd, Hello* h, int* passed) {
    *passed = -1;
    struct iovec iov = {h, sizeof *h};
    struct msghdr m;
    memset(&m, 0, sizeof m);
    m.msg_iov = &iov;
    m.msg_iovlen = 1;
    alignas(struct cmsghdr) char ctl[CMSG_SPACE(sizeof(int) * 4)];
    m.msg_control = ctl;
    m.msg_controllen = sizeof ctl;
    ssize_t k;
    do k = recvmsg(fd, &m, MSG_CMSG_CLOEXEC); while (k < 0 && errno == EINTR);
    if (k <= 0) return false;
    for (struct cmsghdr* c = CMSG_FIRSTHDR(&m); c; c = CMSG_NXTHDR(&m, c)) {
        if (c->cmsg_level != SOL_SOCKET || c->cmsg_type != SCM_RIGHTS) continue;
        const size_t nfd = (c->cmsg_len - CMSG_LEN(0)) / sizeof(int);
        for (size_t i = 0; i < nfd; ++i) {
            int got;
            memcpy(&got, CMSG_DATA(c) + i * sizeof(int), sizeof(int));
            if (*passed < 0) *passed = got;
            else close(got);  // one descriptor is all a client may hand over
        }
    }
    return (size_t)k == sizeof *h || recv_all(fd, (char*)h + k, sizeof *h - (size_t)k);
}

struct Conn {
    int fd = -1, memfd = -1;
    uint8_t* map = nullptr;
    uint64_t map_len = 0;
    ssimu2_ctx* ctx = nullptr;
    RefMirror ref;
    bool erred = false;     // a call of this connection failed: from then on the context's error text is this connection's
    bool batched = false;   // a batch ran: the context keeps its items, so it is destroyed instead of pooled
};

// The client's file, all of it, mapped; false = the request lies about it.
bool remap(Conn* c, uint64_t size) {
    if (size <= c->map_len) return true;
    struct stat st;
    if (size > kShmMax || fstat(c->memfd, &st) != 0 || (uint64_t)st.st_size < size) return false;
    if (c->map) munmap(c->map, c->map_len);
    c->map = nullptr;
    c->map_len = 0;
    void* p = mmap(nullptr, size, PROT_READ | PROT_WRITE, MAP_SHARED, c->memfd, 0);
    if (p == MAP_FAILED) return false;
    c->map = (uint8_t*)p;
    c->map_len = size;
    return true;
}

bool fits(const Conn* c, uint64_t off, uint64_t len) { return off <= c->map_len && len <= c->map_len - off; }

// One request.  false = malformed: the connection is closed, nothing was called.
bool handle(Conn* c, const Request& q, Reply* rep) {
    if (q.magic != kMagic || q.op == 0 || q.op >= kOpCount) return false;
    if (!remap(c, q.shm_size)) return false;
    const Needs n = needs(q, c->ref);
    // a pointer the library will not read (0 bytes) still has to be non-null, and odd where the caller's was
    alignas(2) static const uint8_t kUnread[2] = {0, 0};
    const void* in[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        if (q.in[k].off == kNull) continue;
        if (q.in[k].len != n.in[k] || (n.in[k] && !fits(c, q.in[k].off, n.in[k]))) return false;
        in[k] = n.in[k] ? c->map + q.in[k].off : kUnread + (q.in[k].off & 1u);
    }
    void* out = nullptr;
    if (q.out.off != kNull) {
        if (q.out.len != n.out || (n.out && !fits(c, q.out.off, n.out)) || (q.out.off & 7u)) return false;
        static double unwritten[1];
        out = n.out ? (void*)(c->map + q.out.off) : (void*)unwritten;
    }
    // batches: the offset arrays are copied out of the shared memory before they are checked
    std::vector<const uint8_t*> items[2];
    const bool is_batch = q.op == kOpBatchRgb8 || q.op == kOpBatchRef;
    if (is_batch) {
        const uint64_t item = batch_item_bytes(q, c->ref);
        for (int k = 0; k < 2; ++k) {
            if (!in[k] || !n.in[k]) continue;
            std::vector<uint64_t> offs(q.a[0]);
            memcpy(offs.data(), in[k], n.in[k]);
            items[k].resize(q.a[0]);
            for (uint32_t i = 0; i < q.a[0]; ++i) {
                if (offs[i] == kNull) items[k][i] = nullptr;
                else if (!fits(c, offs[i], item)) return false;
                else items[k][i] = c->map + offs[i];
            }
        }
    }
    memset(rep, 0, sizeof *rep);
    rep->magic = kMagic;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (g_fault) {  // nothing is started on a card after a fault
            rep->rc = SSIMU2_ERR_HIP;
            snprintf(rep->text, sizeof rep->text, "%s", g_fault_text.c_str());
            return true;
        }
    }
    double score = 0.0;
    double* ps = (q.flags & kNoScore) ? nullptr : &score;
    int i0 = 0, rc;
    ssimu2_ctx* x = c->ctx;
    // a null array of a batch stays null; an array the library will not read (n.in == 0) is any non-null pointer
    static const uint8_t* const kNoItems[1] = {nullptr};
    auto arr = [&](int k) -> const uint8_t* const* { return !in[k] ? nullptr : items[k].empty() ? kNoItems : items[k].data(); };
    switch (q.op) {
        case kOpSetBlur: rc = ssimu2_ctx_set_blur(x, (int)q.a[0]); break;
        case kOpScoreRgb8: rc = ssimu2_score_rgb8(x, (const uint8_t*)in[0], (const uint8_t*)in[1], q.a[0], q.a[1], q.a[2], ps); break;
        case kOpSetRef: rc = ssimu2_set_reference(x, (const uint8_t*)in[0], q.a[0], q.a[1]); break;
        case kOpScoreRef: rc = ssimu2_score_against_reference(x, (const uint8_t*)in[0], ps); break;
        case kOpScoreStrided: rc = ssimu2_score_against_reference_strided(x, (const uint8_t*)in[0], q.a[0], q.a[1], ps); break;
        case kOpScoreRgb16:
            rc = ssimu2_score_rgb16(x, (const uint16_t*)in[0], (const uint16_t*)in[1], q.a[0], q.a[1], q.a[2], q.a[3], ps);
            break;
        case kOpSetRef16: rc = ssimu2_set_reference_rgb16(x, (const uint16_t*)in[0], q.a[0], q.a[1], q.a[2]); break;
        case kOpScoreRef16: rc = ssimu2_score_against_reference_rgb16(x, (const uint16_t*)in[0], q.a[0], ps); break;
        case kOpScoreStrided16:
            rc = ssimu2_score_against_reference_strided16(x, (const uint16_t*)in[0], q.a[0], q.a[1], q.a[2], ps);
            break;
        case kOpMapRgb8:
            rc = ssimu2_error_map_rgb8(x, (const uint8_t*)in[0], (const uint8_t*)in[1], q.a[0], q.a[1], q.a[2], (float*)out, ps);
            break;
        case kOpMapRef: rc = ssimu2_error_map_against_reference(x, (const uint8_t*)in[0], (float*)out, ps); break;
        case kOpLastAverages: rc = ssimu2_last_averages(x, (double*)out, &i0); break;
        case kOpBatchRgb8:
            c->batched = true;
            rc = ssimu2_score_batch_rgb8(x, arr(0), arr(1), q.a[0], q.a[1], q.a[2], (double*)out);
            break;
        case kOpBatchRef:
            c->batched = true;
            rc = ssimu2_score_batch_against_reference(x, arr(0), q.a[0], (double*)out);
            break;
        case kOpLastBatchAverages: rc = ssimu2_last_batch_averages(x, q.a[0], (double*)out, &i0); break;
        default: return false;
    }
    c->ref.update(q, rc);
    if (rc != SSIMU2_OK) c->erred = true;
    rep->rc = rc;
    rep->score = score;
    rep->i0 = i0;
    if (c->erred) snprintf(rep->text, sizeof rep->text, "%s", ssimu2_last_error(x));
    if (rc == SSIMU2_ERR_HIP) {
        std::lock_guard<std::mutex> lock(g_mu);
        if (!g_fault) {
            g_fault = true;
            g_fault_at = now();
            g_fault_text = std::string(rep->text) + " (scoring service: a HIP error ended the service; start a new one)";
            fprintf(stderr, "oavif_scored: %s\n", g_fault_text.c_str());
        }
        snprintf(rep->text, sizeof rep->text, "%s", g_fault_text.c_str());
    }
    return true;
}

bool refuse(int fd, int rc, const std::string& why) {
    HelloReply r;
    memset(&r, 0, sizeof r);
    r.magic = kMagic;
    r.rc = rc;
    r.info = g_info;
    snprintf(r.text, sizeof r.text, "%s", why.c_str());
    return send_all(fd, &r, sizeof r);
}

void serve(int fd) {
    Conn c;
    c.fd = fd;
    bool slot = false;
    do {
        struct timeval tv = {5, 0};  // a peer that connects and says nothing does not keep a thread
        (void)setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
        Hello h;
        if (!recv_hello(fd, &h, &c.memfd) || h.magic != kMagic) break;
        tv.tv_sec = 0;
        (void)setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);  // between two calls a client may encode for minutes
        if (h.proto != kProto) {
            refuse(fd, SSIMU2_ERR_NO_DEVICE, "protocol version " + std::to_string(h.proto) + " refused, the service speaks " +
                                                 std::to_string(kProto));
            break;
        }
        if (memchr(h.version, 0, sizeof h.version) == nullptr || strcmp(h.version, ssimu2_version()) != 0) {
            refuse(fd, SSIMU2_ERR_NO_DEVICE, std::string("library version differs from the service's: ") + ssimu2_version());
            break;
        }
        if (!(h.flags & kHelloWantCtx)) {  // ssimu2_query_device
            refuse(fd, SSIMU2_OK, "");
            break;
        }
        const int seals = c.memfd >= 0 ? fcntl(c.memfd, F_GET_SEALS) : -1;
        if (seals < 0 || !(seals & F_SEAL_SHRINK)) {
            refuse(fd, SSIMU2_ERR_NO_DEVICE, "no frame memory passed, or one that may shrink");
            break;
        }
        {
            std::lock_guard<std::mutex> lock(g_mu);
            if (g_fault) {
                refuse(fd, SSIMU2_ERR_HIP, g_fault_text);
                break;
            }
            if (g_active >= g_opt.max_contexts) {
                refuse(fd, SSIMU2_ERR_OOM, "all " + std::to_string(g_opt.max_contexts) +
                                               " contexts of the scoring service are in use (--max-contexts)");
                break;
            }
            ++g_active;
            slot = true;
            if (!g_pool.empty()) {
                c.ctx = g_pool.back();
                g_pool.pop_back();
            }
        }
        if (!c.ctx) {
            const int rc = ssimu2_ctx_create(g_opt.device, nullptr, &c.ctx);
            if (rc != SSIMU2_OK) {
                c.ctx = nullptr;
                refuse(fd, rc, ssimu2_last_error(nullptr));
                break;
            }
        }
        if (!refuse(fd, SSIMU2_OK, "")) break;
        for (;;) {
            Request q;
            Reply rep;
            if (!recv_all(fd, &q, sizeof q)) break;  // closed: the ordinary end
            if (!handle(&c, q, &rep)) {
                fprintf(stderr, "oavif_scored: malformed request (op %u), connection closed\n", q.op);
                break;
            }
            if (!send_all(fd, &rep, sizeof rep)) break;
        }
    } while (false);
    if (c.ctx) {
        // back to the pool as a fresh context: default blur, no reference (ssimu2_ctx_set_blur drops it and frees the
        // recursive modes' planes), nothing pending (nothing is ever enqueued here without its wait)
        bool keep;
        {
            std::lock_guard<std::mutex> lock(g_mu);
            keep = !g_fault && !c.batched;
        }
        if (keep) keep = ssimu2_ctx_set_blur(c.ctx, SSIMU2_BLUR_FIR) == SSIMU2_OK;
        std::unique_lock<std::mutex> lock(g_mu);
        if (keep) {
            g_pool.push_back(c.ctx);
        } else if (!g_fault) {
            lock.unlock();
            ssimu2_ctx_destroy(c.ctx);
            lock.lock();
        }
    }
    if (c.map) munmap(c.map, c.map_len);
    if (c.memfd >= 0) close(c.memfd);
    std::lock_guard<std::mutex> lock(g_mu);
    for (size_t i = 0; i < g_conns.size(); ++i)
        if (g_conns[i] == fd) {
            g_conns.erase(g_conns.begin() + (long)i);
            break;
        }
    close(fd);
    if (slot && --g_active == 0) g_idle_since = now();
    g_cv.notify_all();
}

int usage() {
    fprintf(stderr, "usage: oavif_scored --socket PATH [--device D] [--max-contexts N] [--idle-exit SECONDS] "
                    "[--max-lifetime SECONDS] [--parent-pid PID]\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (i + 1 >= argc) return usage();
        const char* v = argv[++i];
        if (a == "--socket") g_opt.socket = v;
        else if (a == "--device") g_opt.device = atoi(v);
        else if (a == "--max-contexts") g_opt.max_contexts = atoi(v);
        else if (a == "--idle-exit") g_opt.idle_exit = atof(v);
        else if (a == "--max-lifetime") g_opt.max_lifetime = atof(v);
        else if (a == "--parent-pid") g_opt.parent_pid = atol(v);
        else return usage();
    }
    struct sockaddr_un sa;
    memset(&sa, 0, sizeof sa);
    sa.sun_family = AF_UNIX;
    if (g_opt.socket.empty() || g_opt.socket.size() >= sizeof sa.sun_path || g_opt.max_contexts < 1) return usage();
    memcpy(sa.sun_path, g_opt.socket.c_str(), g_opt.socket.size());

    struct sigaction act;
    memset(&act, 0, sizeof act);
    act.sa_handler = on_signal;
    sigaction(SIGTERM, &act, nullptr);
    sigaction(SIGINT, &act, nullptr);
    signal(SIGPIPE, SIG_IGN);
    if (g_opt.parent_pid > 0) {  // no GPU process outlives the job that started it
        prctl(PR_SET_PDEATHSIG, SIGTERM);
        if ((long)getppid() != g_opt.parent_pid) {
            fprintf(stderr, "oavif_scored: parent %ld is gone\n", g_opt.parent_pid);
            return 0;
        }
    }

    // a live socket is not stolen, a stale one is replaced
    {
        const int probe = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
        if (probe < 0) {
            perror("oavif_scored: socket");
            return 1;
        }
        const bool live = connect(probe, (struct sockaddr*)&sa, sizeof sa) == 0;
        close(probe);
        if (live) {
            fprintf(stderr, "oavif_scored: %s is the socket of a running service\n", g_opt.socket.c_str());
            return 2;
        }
        struct stat st;
        if (lstat(g_opt.socket.c_str(), &st) == 0) {
            if (!S_ISSOCK(st.st_mode)) {
                fprintf(stderr, "oavif_scored: %s exists and is not a socket\n", g_opt.socket.c_str());
                return 2;
            }
            unlink(g_opt.socket.c_str());
        }
    }
    const int lfd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    const mode_t old_umask = umask(0177);  // the file is born 0600
    if (lfd < 0 || bind(lfd, (struct sockaddr*)&sa, sizeof sa) != 0 || listen(lfd, 64) != 0) {
        perror("oavif_scored: bind");
        return 1;
    }
    umask(old_umask);
    chmod(g_opt.socket.c_str(), 0600);

    // the HIP context of the one device, before anybody is told the service is ready
    ssimu2_ctx* first = nullptr;
    const int rc = ssimu2_ctx_create(g_opt.device, nullptr, &first);
    if (rc != SSIMU2_OK) {
        fprintf(stderr, "oavif_scored: ssimu2_ctx_create(%d) = %d: %s\n", g_opt.device, rc, ssimu2_last_error(nullptr));
        unlink(g_opt.socket.c_str());
        return 1;
    }
    memset(&g_info, 0, sizeof g_info);
    g_info.struct_size = (uint32_t)sizeof g_info;
    (void)ssimu2_ctx_device_info(first, &g_info);
    g_pool.push_back(first);
    const double t0 = now();
    g_idle_since = t0;
    printf("ready %s %s\n", g_opt.socket.c_str(), ssimu2_version());
    fflush(stdout);

    const char* why = "";
    int code = 0;
    for (;;) {
        struct pollfd p = {lfd, POLLIN, 0};
        const int k = poll(&p, 1, 100);
        const double t = now();
        if (g_signal) { why = "signal"; break; }
        if (g_opt.parent_pid > 0 && (long)getppid() != g_opt.parent_pid) { why = "parent gone"; break; }
        if (g_opt.max_lifetime > 0 && t - t0 >= g_opt.max_lifetime) { why = "--max-lifetime"; break; }
        {
            std::lock_guard<std::mutex> lock(g_mu);
            if (g_fault && (g_active == 0 || t - g_fault_at >= 5.0)) { why = "HIP error"; code = 3; break; }
            if (g_opt.idle_exit > 0 && g_active == 0 && g_conns.empty() && t - g_idle_since >= g_opt.idle_exit) { why = "--idle-exit"; break; }
        }
        if (k <= 0 || !(p.revents & POLLIN)) continue;
        const int fd = accept4(lfd, nullptr, nullptr, SOCK_CLOEXEC);
        if (fd < 0) continue;
        struct ucred cred;
        socklen_t len = sizeof cred;
        if (getsockopt(fd, SOL_SOCKET, SO_PEERCRED, &cred, &len) != 0 || cred.uid != geteuid()) {
            close(fd);  // another user's process: dropped before anything is read
            continue;
        }
        {
            std::lock_guard<std::mutex> lock(g_mu);
            g_conns.push_back(fd);
            g_idle_since = t;
        }
        try {
            std::thread(serve, fd).detach();
        } catch (...) {
            std::lock_guard<std::mutex> lock(g_mu);
            g_conns.pop_back();
            close(fd);
        }
    }
    // orderly exit: no new connections, the socket file gone, live connections cut after their current call
    close(lfd);
    unlink(g_opt.socket.c_str());
    fprintf(stderr, "oavif_scored: leaving (%s)\n", why);
    bool drained;
    {
        std::unique_lock<std::mutex> lock(g_mu);
        for (int fd : g_conns) shutdown(fd, SHUT_RDWR);
        drained = g_cv.wait_for(lock, std::chrono::seconds(5), [] { return g_conns.empty(); });
    }
    if (!drained || code != 0) _exit(code);  // a call still on the GPU, or a faulted card: nothing more is touched
    for (ssimu2_ctx* x : g_pool) ssimu2_ctx_destroy(x);
    g_pool.clear();
    return 0;
}
