// Wave placement probe for gfx950: which SIMD each wave of an 8-wave workgroup lands on, in
// k_march's launch shape (512 threads, __launch_bounds__(512, 6), ~50 KB of LDS, so three
// workgroups share a CU).  Every wave reads HW_REG_HW_ID (SIMD id, CU, workgroup slot) and
// HW_REG_XCC_ID once and lane 0 writes them with an ordinary vector store; then the wave runs a
// VALU loop of ~20 us so that the workgroups of a CU are resident together.
// Output: how the SIMD of wave w is distributed, whether simd == (w + k) mod 4 holds per workgroup,
// and the SIMDs of waves 0-1 (k_march's converter waves) per CU, counted over the three
// co-resident workgroups.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <string>
#include <map>
#include <vector>

constexpr int THREADS = 512, WAVES = THREADS / 64;
constexpr int LDS_FLOATS = 50 * 1024 / 4;
// s_getreg_b32 immediates: id | offset << 6 | (size - 1) << 11
constexpr int HWREG_HW_ID = 4 | (31 << 11);
constexpr int HWREG_XCC_ID = 20 | (31 << 11);

struct Rec {
    unsigned hw_id, xcc_id, t0_lo, t0_hi;
};

__global__ __launch_bounds__(THREADS, 6) void k_probe(Rec* out, float* sink, int iters) {
    __shared__ float lds[LDS_FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned hw = __builtin_amdgcn_s_getreg(HWREG_HW_ID);
    const unsigned xcc = __builtin_amdgcn_s_getreg(HWREG_XCC_ID);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        Rec r{hw, xcc, (unsigned)t0, (unsigned)(t0 >> 32)};
        out[blockIdx.x * WAVES + wave] = r;
    }
    for (int i = threadIdx.x; i < LDS_FLOATS; i += THREADS) lds[i] = (float)i;
    __syncthreads();
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = lds[(threadIdx.x * 8 + j) % LDS_FLOATS];
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = fmaf(x[j], 0.999f, 0.5f);
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j];
    if (s == 12345.0f) sink[threadIdx.x] = s;  // keeps the loop; never true in practice
}

int main(int argc, char** argv) {
    const int nblocks = argc > 1 ? atoi(argv[1]) : 1536;
    const int iters = argc > 2 ? atoi(argv[2]) : 20000;
    Rec* d_out;
    float* d_sink;
    hipMalloc(&d_out, sizeof(Rec) * nblocks * WAVES);
    hipMalloc(&d_sink, sizeof(float) * THREADS);
    hipMemset(d_out, 0, sizeof(Rec) * nblocks * WAVES);
    hipFuncAttributes fa;
    hipFuncGetAttributes(&fa, (const void*)k_probe);
    int per_cu = 0;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_probe, THREADS, 0);
    k_probe<<<nblocks, THREADS>>>(d_out, d_sink, iters);
    if (hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "kernel failed\n");
        return 1;
    }
    std::vector<Rec> r((size_t)nblocks * WAVES);
    hipMemcpy(r.data(), d_out, sizeof(Rec) * r.size(), hipMemcpyDeviceToHost);
    printf("k_probe: %d workgroups of %d threads, %d VGPRs (arch), %zu B LDS, %d workgroups/CU (occupancy API)\n",
           nblocks, THREADS, fa.numRegs, fa.sharedSizeBytes, per_cu);

    auto simd = [](unsigned h) { return (h >> 4) & 3u; };
    auto slot = [](unsigned h) { return (h >> 16) & 15u; };
    auto cu_key = [](const Rec& x) { return ((unsigned long long)x.xcc_id << 32) | (x.hw_id & 0xFF00u); };  // XCC, SE, SH, CU
    // 1. SIMD of wave w
    long hist[WAVES][4] = {};
    // 2. per workgroup: offset k with simd(w) == (w + k) mod 4 for every w, or -1
    long offs[5] = {};
    long per_simd_count[5] = {};  // waves of one workgroup per SIMD: histogram of the max
    std::map<unsigned, long> slot_hist;
    std::map<unsigned, std::array<long, 4>> off_by_slot;
    for (int b = 0; b < nblocks; ++b) {
        const Rec* w = &r[(size_t)b * WAVES];
        int cnt[4] = {};
        for (int i = 0; i < WAVES; ++i) {
            hist[i][simd(w[i].hw_id)]++;
            cnt[simd(w[i].hw_id)]++;
        }
        int mx = 0;
        for (int s = 0; s < 4; ++s) mx = cnt[s] > mx ? cnt[s] : mx;
        per_simd_count[mx > 4 ? 4 : mx]++;
        int k = ((int)simd(w[0].hw_id)) & 3;
        for (int i = 0; i < WAVES; ++i)
            if ((int)simd(w[i].hw_id) != ((i + k) & 3)) k = -1;
        if (k < 0) offs[4]++;
        else offs[k]++;
        const unsigned sl = slot(w[0].hw_id);
        slot_hist[sl]++;
        if (k >= 0) off_by_slot[sl][k]++;
    }
    printf("\nSIMD of wave w (counts over all workgroups):\n");
    for (int i = 0; i < WAVES; ++i)
        printf("  wave %d: simd0 %6ld  simd1 %6ld  simd2 %6ld  simd3 %6ld\n", i, hist[i][0], hist[i][1], hist[i][2], hist[i][3]);
    printf("\nworkgroups with simd(w) == (w + k) mod 4 for all w:  k=0 %ld  k=1 %ld  k=2 %ld  k=3 %ld  none %ld\n",
           offs[0], offs[1], offs[2], offs[3], offs[4]);
    printf("most waves of one workgroup on one SIMD:  1: %ld  2: %ld  3: %ld  >=4: %ld\n", per_simd_count[1],
           per_simd_count[2], per_simd_count[3], per_simd_count[4]);
    std::map<std::string, long> patterns;  // SIMD of waves 0..7
    for (int b = 0; b < nblocks; ++b) {
        std::string p_;
        for (int i = 0; i < WAVES; ++i) p_ += std::to_string(simd(r[(size_t)b * WAVES + i].hw_id));
        patterns[p_ + " slot " + std::to_string(slot(r[(size_t)b * WAVES].hw_id))]++;
    }
    printf("\nSIMDs of waves 0..7 and the workgroup slot:\n");
    for (auto& kv : patterns) printf("  %s: %ld\n", kv.first.c_str(), kv.second);
    printf("\nworkgroup slot (HW_ID TG_ID) of wave 0, and the offset k by slot:\n");
    for (auto& kv : slot_hist) {
        auto& o = off_by_slot[kv.first];
        printf("  slot %2u: %6ld workgroups   k=0 %ld k=1 %ld k=2 %ld k=3 %ld\n", kv.first, kv.second, o[0], o[1], o[2], o[3]);
    }
    // 3. co-resident workgroups: the first wave of the launch on each CU ran in the first wave of
    // dispatch; the workgroups that started within 2 us of the CU's first start were resident together.
    std::map<unsigned long long, std::vector<int>> by_cu;
    for (int b = 0; b < nblocks; ++b) by_cu[cu_key(r[(size_t)b * WAVES])].push_back(b);
    long conv_hist[7][4] = {};  // converters (waves 0-1) per SIMD on one CU, first resident set
    long cus = 0, max_load[7] = {};
    std::map<std::string, long> slot_sets;  // workgroup slots of the first resident set
    std::map<std::string, long> spread;     // waves 0-1 of the first resident set per SIMD, largest first
    for (auto& kv : by_cu) {
        auto& v = kv.second;
        unsigned long long tmin = ~0ull;
        for (int b : v) {
            const Rec& x = r[(size_t)b * WAVES];
            unsigned long long t = ((unsigned long long)x.t0_hi << 32) | x.t0_lo;
            tmin = t < tmin ? t : tmin;
        }
        int conv[4] = {}, nwg = 0;
        std::vector<unsigned> slots;
        for (int b : v) {
            const Rec* w = &r[(size_t)b * WAVES];
            unsigned long long t = ((unsigned long long)w[0].t0_hi << 32) | w[0].t0_lo;
            if (t - tmin > 200) continue;  // the real-time counter runs at 100 MHz: 2 us
            ++nwg;
            slots.push_back(slot(w[0].hw_id));
            conv[simd(w[0].hw_id)]++;
            conv[simd(w[1].hw_id)]++;
        }
        if (nwg > 6) nwg = 6;
        int mx = 0;
        for (int s = 0; s < 4; ++s) mx = conv[s] > mx ? conv[s] : mx;
        for (int s = 0; s < 4; ++s) conv_hist[nwg][s] += conv[s];
        max_load[mx > 6 ? 6 : mx]++;
        int sorted_[4] = {conv[0], conv[1], conv[2], conv[3]};
        std::sort(sorted_, sorted_ + 4);
        spread[std::to_string(sorted_[3]) + "/" + std::to_string(sorted_[2]) + "/" + std::to_string(sorted_[1]) + "/" +
               std::to_string(sorted_[0])]++;
        std::sort(slots.begin(), slots.end());
        std::string key;
        for (unsigned x : slots) key += std::to_string(x) + " ";
        slot_sets[key]++;
        ++cus;
    }
    printf("\nfirst resident set per CU (%ld CUs): waves 0-1 of its workgroups per SIMD, summed over CUs:\n", cus);
    for (int n = 1; n <= 6; ++n)
        if (conv_hist[n][0] + conv_hist[n][1] + conv_hist[n][2] + conv_hist[n][3])
            printf("  CUs with %d resident workgroups: simd0 %ld simd1 %ld simd2 %ld simd3 %ld\n", n, conv_hist[n][0],
                   conv_hist[n][1], conv_hist[n][2], conv_hist[n][3]);
    printf("  most of those waves on one SIMD of a CU: ");
    for (int m = 0; m <= 6; ++m) printf("%d: %ld  ", m, max_load[m]);
    printf("\n  spread of those waves over the four SIMDs (largest first):");
    for (auto& kv : spread) printf("  %s: %ld CUs", kv.first.c_str(), kv.second);
    printf("\n  workgroup slots of the first resident set:");
    for (auto& kv : slot_sets) printf("  {%s}: %ld", kv.first.c_str(), kv.second);
    printf("\n");
    hipFree(d_out);
    hipFree(d_sink);
    return 0;
}
