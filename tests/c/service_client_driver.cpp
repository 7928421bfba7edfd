// TEST INFRASTRUCTURE -- a stand-alone driver of oavif_amd/csrc/remote_client.cpp (the client side of the scoring
// service) for the sanitizer runs of tests/test_service_cpu.py: `threads` concurrent clients of the service at
// OAVIF_SCORER_SOCKET, each with a context of its own, `rounds` times: pair score, cached reference, strided RGBA
// from ssimu2_host_alloc memory, 16-bit, a map, a batch, the averages.  Every score is held to the stand-in scorer's
// formula (tests/c/stub_scorer_full.c).  Exit 0 = all equal.
//   service_client_driver VERSION threads rounds
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "remote_client.h"

using namespace ssimu2r;

static std::atomic<int> g_bad{0};
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "line %d: %s failed (%s)\n", __LINE__, #cond, r ? last_error(r) : ""); \
            ++g_bad;                                                           \
            if (r) destroy(r);                                                 \
            return;                                                            \
        }                                                                      \
    } while (0)

static double formula(const uint8_t* a, const uint8_t* b, uint32_t w, uint32_t h) {
    unsigned long long sad = 0;
    for (size_t i = 0; i < (size_t)w * h * 3; ++i) sad += (unsigned)abs((int)a[i] - (int)b[i]);
    return 100.0 - 6.0 * (double)sad / ((double)w * h * 3);
}

static void client(const char* version, int id, int rounds) {
    Remote* r = nullptr;
    ssimu2_device_info info;
    std::string err;
    const int rc = create(0, nullptr, version, &r, &info, &err);
    if (rc != SSIMU2_OK) {
        fprintf(stderr, "create: %d %s\n", rc, err.c_str());
        ++g_bad;
        return;
    }
    for (int round = 0; round < rounds; ++round) {
        const uint32_t w = 37 + 13 * (uint32_t)id + (uint32_t)round, h = 21 + (uint32_t)id;
        std::vector<uint8_t> a((size_t)w * h * 3), b(a.size());
        unsigned s = 1234u * (unsigned)(id + 1) + (unsigned)round;
        for (size_t i = 0; i < a.size(); ++i) {
            s = s * 1664525u + 1013904223u;
            a[i] = (uint8_t)(s >> 24);
            b[i] = (uint8_t)(s >> 16);
        }
        const double want = formula(a.data(), b.data(), w, h);
        double got = 0;
        CHECK(score_rgb8(r, a.data(), b.data(), w, h, 3, &got) == SSIMU2_OK && got == want);
        CHECK(score_against_reference(r, b.data(), &got) == SSIMU2_ERR_NO_REFERENCE);
        CHECK(set_reference(r, a.data(), w, h) == SSIMU2_OK);
        CHECK(score_against_reference(r, b.data(), &got) == SSIMU2_OK && got == want);
        void* mem = nullptr;
        const uint32_t row = w * 4 + 12;
        CHECK(host_alloc(r, (size_t)row * h, &mem) == SSIMU2_OK);
        uint8_t* rgba = (uint8_t*)mem;
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x)
                for (int k = 0; k < 3; ++k) rgba[(size_t)y * row + x * 4 + k] = b[((size_t)y * w + x) * 3 + k];
        CHECK(score_strided(r, rgba, row, 4, &got) == SSIMU2_OK && got == want);
        CHECK(host_free(r, mem) == SSIMU2_OK);
        std::vector<uint16_t> b16(a.size());
        for (size_t i = 0; i < a.size(); ++i) b16[i] = (uint16_t)(b[i] * 257u);
        CHECK(score_against_reference_rgb16(r, b16.data(), 16, &got) == SSIMU2_OK);
        std::vector<float> map((size_t)w * h);
        CHECK(error_map_against_reference(r, b.data(), map.data(), &got) == SSIMU2_OK && got == want);
        double avg[108];
        int ns = 0;
        CHECK(last_averages(r, avg, &ns) == SSIMU2_OK && avg[107] == want + 107);
        const uint8_t* items[3] = {b.data(), a.data(), b.data()};
        double scores[3];
        CHECK(score_batch_against_reference(r, items, 3, scores) == SSIMU2_OK && scores[0] == want && scores[1] == 100.0);
        CHECK(set_blur(r, SSIMU2_BLUR_RECURSIVE) == SSIMU2_OK);
        CHECK(score_batch_against_reference(r, items, 3, scores) == SSIMU2_ERR_UNSUPPORTED);
        CHECK(set_blur(r, SSIMU2_BLUR_FIR) == SSIMU2_OK);
    }
    destroy(r);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int threads = atoi(argv[2]), rounds = atoi(argv[3]);
    std::vector<std::thread> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(client, argv[1], i, rounds);
    for (auto& t : pool) t.join();
    if (g_bad) fprintf(stderr, "%d client(s) failed\n", g_bad.load());
    return g_bad ? 1 : 0;
}
