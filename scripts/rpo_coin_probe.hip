// Kernel timings of the RPO-256 public coin on one MI355X (hipEvents, resident data, warm), driven by scripts/rpo_coin_probe.py:
//   chain    one rpo_coin_step launch that draws 512 words from a coin with nothing unread = 64 dependent permutations, in the
//            lane-per-element form the library launches (Wide) and in the one-lane form of the same kernel (Narrow)
//   search   rpo_coin_pow_grind over a full window of 2^24 nonces (bits = 63: nothing is found, every lane runs its permutation) against
//            rpo256_merge_level on 2^24 nodes: the same per-lane arithmetic, with and without the loads
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/rpo_coin_probe.hip -o scripts/rpo_coin_probe_bin
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../ministark_amd/csrc/rpo_coin_kernels.h"

#define CHK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("FAILED: %s: %s (line %d)\n", #e, hipGetErrorString(r_), __LINE__); return 1; } } while (0)

using msrpocoin::State;

template <class Launch>
static int median_us(Launch launch, int warm, int reps, double* out) {
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    std::vector<double> t;
    for (int r = 0; r < warm + reps; r++) {
        CHK(hipEventRecord(e0, 0));
        launch();
        CHK(hipEventRecord(e1, 0));
        CHK(hipEventSynchronize(e1));
        CHK(hipGetLastError());
        float ms = 0;
        CHK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= warm) t.push_back(ms * 1e3);
    }
    std::sort(t.begin(), t.end());
    *out = t[t.size() / 2];
    CHK(hipEventDestroy(e0)); CHK(hipEventDestroy(e1));
    return 0;
}

int main() {
    const int PERMS = 64;
    const size_t words = (size_t)PERMS * 8;
    State h;
    for (int q = 0; q < 12; q++) h.s[q] = 1000003ull * (q + 1);
    h.pos = 12;
    for (int q = 0; q < 7; q++) h.pad[q] = 0;
    State* d_coin = nullptr;
    uint64_t *d_out = nullptr, *d_ref = nullptr;
    CHK(hipMalloc(&d_coin, sizeof(State)));
    CHK(hipMalloc(&d_out, words * 8)); CHK(hipMalloc(&d_ref, words * 8));
    auto reset = [&]() { return hipMemcpy(d_coin, &h, sizeof h, hipMemcpyHostToDevice); };
    // the two forms write the same words
    CHK(reset());
    hipLaunchKernelGGL((msrpocoin::rpo_coin_step<msrpocoin::Wide, msrpocoin::OP_DRAW>), dim3(1), dim3(msrpocoin::WAVE), 0, 0, d_coin, nullptr, 0, words, d_out);
    CHK(reset());
    hipLaunchKernelGGL((msrpocoin::rpo_coin_step<msrpocoin::Narrow, msrpocoin::OP_DRAW>), dim3(1), dim3(msrpocoin::WAVE), 0, 0, d_coin, nullptr, 0, words, d_ref);
    std::vector<uint64_t> a(words), b(words);
    CHK(hipMemcpy(a.data(), d_out, words * 8, hipMemcpyDeviceToHost)); CHK(hipMemcpy(b.data(), d_ref, words * 8, hipMemcpyDeviceToHost));
    if (a != b) { printf("FAILED: the two forms of the chain disagree\n"); return 1; }
    double wide = 0, narrow = 0;
    CHK(reset());
    if (median_us([&]() { hipLaunchKernelGGL((msrpocoin::rpo_coin_step<msrpocoin::Wide, msrpocoin::OP_DRAW>), dim3(1), dim3(msrpocoin::WAVE), 0, 0, d_coin, nullptr, 0, words, d_out); }, 3, 15, &wide)) return 1;
    CHK(reset());
    if (median_us([&]() { hipLaunchKernelGGL((msrpocoin::rpo_coin_step<msrpocoin::Narrow, msrpocoin::OP_DRAW>), dim3(1), dim3(msrpocoin::WAVE), 0, 0, d_coin, nullptr, 0, words, d_ref); }, 3, 15, &narrow)) return 1;
    printf("chain: one draw of %zu words = %d dependent permutations, median of 15\n", words, PERMS);
    printf("  lane-per-element (shipped)  %9.1f us per launch  %7.2f us per permutation\n", wide, wide / PERMS);
    printf("  one lane                    %9.1f us per launch  %7.2f us per permutation\n", narrow, narrow / PERMS);
    printf("  one lane / lane-per-element %9.2f\n", narrow / wide);

    const size_t N = (size_t)1 << 24;
    uint64_t *d_src = nullptr, *d_dst = nullptr;
    unsigned long long* d_found = nullptr;
    CHK(hipMalloc(&d_src, N * 64)); CHK(hipMalloc(&d_dst, N * 32)); CHK(hipMalloc(&d_found, 8));
    CHK(hipMemset(d_src, 0x5a, N * 64));                      // words 0x5a5a...: below p
    CHK(hipMemset(d_found, 0xff, 8));
    CHK(reset());
    const dim3 grid((unsigned)(N / msrpocoin::NT)), block(msrpocoin::NT);
    double grind = 0, merge = 0;
    for (int round = 0; round < 2; round++) {                 // alternate, keep the second round
        if (median_us([&]() { hipLaunchKernelGGL(msrpocoin::rpo_coin_pow_grind, grid, block, 0, 0, (const State*)d_coin, 1ull, (unsigned long long)N, 63u, d_found); }, 1, 5, &grind)) return 1;
        if (median_us([&]() { hipLaunchKernelGGL(msrpo::rpo256_merge_level, grid, block, 0, 0, (const uint64_t*)d_src, d_dst, N); }, 1, 5, &merge)) return 1;
    }
    printf("search: 2^24 permutations per launch, median of 5\n");
    printf("  rpo_coin_pow_grind          %9.1f us  %8.1f M permutations/s\n", grind, N / grind);
    printf("  rpo256_merge_level          %9.1f us  %8.1f M permutations/s\n", merge, N / merge);
    printf("  search rate / merge rate    %9.3f\n", merge / grind);
    return 0;
}
