// Host code and kernels of the row sort (ministark_amd/csrc/ms_sort.cpp, sort_kernels.h) under AddressSanitizer and UBSan, as a stand-alone
// CPU program: its own main, linked with the simulator build of the library's sources, where device memory is malloc'd memory and a slot of
// the scatter, a histogram entry or a gathered row out of range is a heap overflow the sanitizer sees.  It runs ms_sort_rows over the lengths
// 0, 1, 2, T+1, 2T+1 (T = 2048, the rows of a tile), 1 .. 4 key components, both fields and the three masks, compares every
// Goldilocks result with std::stable_sort on the canonical values (the 252-bit results: a permutation with the inactive rows behind, in
// order), applies it with ms_permute_columns, gathers through an index with entries past the source, and tries the refusals; then prints
// "sort sanitize ok".  Not part of the suite (the build compiles every translation unit again); from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/sort_sanitize.cpp -o sort_sanitize -ldl && ./sort_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../include/ministark_hip_sort.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

static uint64_t lcg = 11;
static uint64_t next(uint64_t bound) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (lcg >> 33) % bound; }

// the canonical value of a Goldilocks Montgomery word: w 2^-64 = w 2^128 (2^192 = 1 mod p)
static uint64_t gl_canon(uint64_t w) {
    const unsigned __int128 p = 0xFFFFFFFF00000001ull, r2 = 18446744065119617025ull;
    return (uint64_t)((unsigned __int128)(w % (uint64_t)p) * r2 % p);
}

static int run(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned nkeys, int mask) {
    const unsigned nbase = nkeys + 1, mask_col = nkeys;
    std::vector<std::vector<uint64_t>> host(nbase, std::vector<uint64_t>(n * V, 0));
    // a word below 2^32 is below p in both fields, so canonical as a residue; the leading components take few values, so rows tie
    for (unsigned c = 0; c < nbase; c++) for (size_t i = 0; i < n; i++) host[c][i * V + (c % V)] = next(c == mask_col ? 2 : c + 1 < nkeys ? 3 : 1u << 31);
    std::vector<void*> dev(nbase, nullptr), out(nbase, nullptr);
    for (unsigned c = 0; c < nbase; c++) {
        REQUIRE(ms_alloc(ctx, n * V * 8 ? n * V * 8 : 8, &dev[c]) == MS_OK);
        REQUIRE(ms_alloc(ctx, n * V * 8 ? n * V * 8 : 8, &out[c]) == MS_OK);
        if (n) REQUIRE(ms_upload(ctx, dev[c], host[c].data(), n * V * 8) == MS_OK);
    }
    void *d_perm = nullptr, *d_report = nullptr;
    REQUIRE(ms_alloc(ctx, n * 4 ? n * 4 : 8, &d_perm) == MS_OK);
    REQUIRE(ms_alloc(ctx, sizeof(ms_sort_report), &d_report) == MS_OK);
    ms_sort_key key = {{0, 0, 0, 0}, mask, (int32_t)mask_col, 0, 0};
    for (unsigned c = 0; c < nkeys; c++) key.cols[c] = (int32_t)c;
    REQUIRE(ms_sort_rows(ctx, field, n, dev.data(), nbase, nkeys, &key, d_perm, d_report) == MS_OK);
    std::vector<uint32_t> perm(n);
    ms_sort_report rep;
    if (n) REQUIRE(ms_download(ctx, perm.data(), d_perm, n * 4) == MS_OK);
    REQUIRE(ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
    auto is_active = [&](size_t i) { bool zero = true; for (unsigned l = 0; l < V; l++) zero = zero && host[mask_col][i * V + l] == 0; return mask == MS_EXT_ALWAYS || zero == (mask == MS_EXT_IF_ZERO); };
    std::vector<uint32_t> act, ina;
    for (size_t i = 0; i < n; i++) (is_active(i) ? act : ina).push_back((uint32_t)i);
    REQUIRE(rep.active == act.size());
    REQUIRE(std::equal(ina.begin(), ina.end(), perm.begin() + (n ? act.size() : 0)));      // the inactive rows behind, in their order
    std::vector<uint32_t> head(perm.begin(), perm.begin() + act.size()), seen = head;
    std::sort(seen.begin(), seen.end());
    REQUIRE(seen == act);                                                                  // a permutation of the active rows
    if (V == 1) {
        std::stable_sort(act.begin(), act.end(), [&](uint32_t a, uint32_t b) {
            for (unsigned c = 0; c < nkeys; c++) { const uint64_t x = gl_canon(host[c][a]), y = gl_canon(host[c][b]); if (x != y) return x < y; }
            return false;
        });
        REQUIRE(head == act);
    }
    // apply it
    if (n) {
        REQUIRE(ms_permute_columns(ctx, field, n, dev.data(), out.data(), nbase, d_perm, n) == MS_OK);
        std::vector<uint64_t> got(n * V);
        for (unsigned c = 0; c < nbase; c++) {
            REQUIRE(ms_download(ctx, got.data(), out[c], n * V * 8) == MS_OK);
            for (size_t i = 0; i < n; i++) for (unsigned l = 0; l < V; l++) REQUIRE(got[i * V + l] == host[c][(size_t)perm[i] * V + l]);
        }
        // an index with entries past the source: zero elements, nothing read
        std::vector<uint32_t> wild(n);
        for (size_t i = 0; i < n; i++) wild[i] = i % 3 == 0 ? (uint32_t)(n + next(1u << 31)) : (uint32_t)next(n);
        wild[0] = 0xFFFFFFFFu;
        REQUIRE(ms_upload(ctx, d_perm, wild.data(), n * 4) == MS_OK);
        REQUIRE(ms_permute_columns(ctx, field, n, dev.data(), out.data(), 1, d_perm, n) == MS_OK);
        REQUIRE(ms_download(ctx, got.data(), out[0], n * V * 8) == MS_OK);
        for (size_t i = 0; i < n; i++) for (unsigned l = 0; l < V; l++) REQUIRE(got[i * V + l] == (wild[i] < n ? host[0][(size_t)wild[i] * V + l] : 0));
        // refusals leave before anything is enqueued
        REQUIRE(ms_sort_rows(ctx, field, n, dev.data(), nbase, nkeys, &key, dev[0], d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
        REQUIRE(ms_permute_columns(ctx, field, n, dev.data(), dev.data(), 1, d_perm, n) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
        ms_sort_key bad = key;
        bad.cols[nkeys - 1] = (int32_t)nbase;
        REQUIRE(ms_sort_rows(ctx, field, n, dev.data(), nbase, nkeys, &bad, d_perm, d_report) == MS_ERR_INVALID);
    }
    REQUIRE(ms_sort_rows(ctx, field, n, dev.data(), nbase, 0, &key, d_perm, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_sort_rows(ctx, field, n, dev.data(), nbase, MS_SORT_MAX_KEYS + 1, &key, d_perm, d_report) == MS_ERR_INVALID);
    for (void* p : dev) REQUIRE(ms_free(ctx, p) == MS_OK);
    for (void* p : out) REQUIRE(ms_free(ctx, p) == MS_OK);
    REQUIRE(ms_free(ctx, d_perm) == MS_OK);
    REQUIRE(ms_free(ctx, d_report) == MS_OK);
    return 0;
}

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const size_t T = 2048, lengths[] = {0, 1, 2, T + 1, 2 * T + 1};
    unsigned k = 0;
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (size_t n : lengths)
            for (unsigned twice = 0; twice < 2; twice++, k++)                              // 1 .. 4 components and the three masks go round
                if (run(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, n, 1 + k % MS_SORT_MAX_KEYS, (int)(k % 3))) return 1;
    for (int checked = 0; checked < 2; checked++) {                    // and once in checked mode, which scans the named columns first
        REQUIRE(ms_ctx_set_checked(ctx, checked) == MS_OK);
        if (run(ctx, MS_GOLDILOCKS_FP, 1, 300, 2, MS_EXT_IF_NONZERO)) return 1;
    }
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("sort sanitize ok\n");
    fflush(stdout);
    return 0;
}
