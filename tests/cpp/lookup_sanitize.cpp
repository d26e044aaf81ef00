// Host code and kernels of the lookup multiplicities (ministark_amd/csrc/ms_lookup.cpp, lookup_kernels.h) under AddressSanitizer and UBSan,
// as a stand-alone CPU program: its own main, linked with the simulator build of the library's sources, where device memory is malloc'd
// memory and a slot, counter or column index out of range is a heap overflow the sanitizer sees.  It runs ms_lookup_multiplicities over
// lengths 0 .. 1025, widths 1 .. 4, both fields, masks, 0 .. 8 sets, m in place, and its refusals, compares every result with a std::map,
// and prints "lookup sanitize ok".  Not part of the suite (the build compiles every translation unit again); from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/lookup_sanitize.cpp -o lookup_sanitize -ldl && ./lookup_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>
#include "../../include/ministark_hip_lookup.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

static uint64_t lcg = 7;
static uint64_t next(uint64_t bound) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (lcg >> 33) % bound; }

// one call on small values v (the element is the words {v, 0, ..}: below p in both fields, so canonical) against a map
static int run(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned width, unsigned nsets, int table_mask, int lookup_mask) {
    const unsigned nbase = width * (1 + nsets) + 2;                  // the tuples' columns, a mask column, the m column
    const unsigned mask_col = nbase - 2, m_col = nbase - 1;
    std::vector<std::vector<uint64_t>> host(nbase, std::vector<uint64_t>(n * V, 0));
    for (unsigned c = 0; c < nbase - 1; c++) for (size_t i = 0; i < n; i++) host[c][i * V + (c % V)] = next(c == mask_col ? 2 : 3);
    std::vector<void*> dev(nbase, nullptr);
    for (unsigned c = 0; c < nbase; c++) {
        REQUIRE(ms_alloc(ctx, n * V * 8 ? n * V * 8 : 8, &dev[c]) == MS_OK);
        if (n) REQUIRE(ms_upload(ctx, dev[c], host[c].data(), n * V * 8) == MS_OK);
    }
    void* d_report = nullptr;
    REQUIRE(ms_alloc(ctx, sizeof(ms_lookup_report), &d_report) == MS_OK);
    ms_lookup_tuple table = {{0, 0, 0, 0}, table_mask, (int32_t)mask_col, 0, 0};
    std::vector<ms_lookup_tuple> sets(nsets, ms_lookup_tuple{{0, 0, 0, 0}, lookup_mask, (int32_t)mask_col, 0, 0});
    for (unsigned c = 0; c < width; c++) { table.cols[c] = (int32_t)c; for (unsigned s = 0; s < nsets; s++) sets[s].cols[c] = (int32_t)(width * (1 + s) + c); }
    REQUIRE(ms_lookup_multiplicities(ctx, field, n, dev.data(), nbase, width, &table, nsets ? sets.data() : nullptr, nsets, dev[m_col], d_report) == MS_OK);
    std::vector<uint64_t> got(n * V);
    ms_lookup_report rep;
    if (n) REQUIRE(ms_download(ctx, got.data(), dev[m_col], n * V * 8) == MS_OK);
    REQUIRE(ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
    auto is_active = [&](int kind, size_t i) { bool zero = true; for (unsigned l = 0; l < V; l++) zero = zero && host[mask_col][i * V + l] == 0; return kind == MS_EXT_ALWAYS || zero == (kind == MS_EXT_IF_ZERO); };
    auto key = [&](unsigned c0, size_t i) { std::vector<uint64_t> k; for (unsigned c = 0; c < width; c++) for (unsigned l = 0; l < V; l++) k.push_back(host[c0 + c][i * V + l]); return k; };
    std::map<std::vector<uint64_t>, size_t> first;
    uint64_t dups = 0, missing = 0, first_set = 0, first_row = 0;
    for (size_t j = 0; j < n; j++) if (is_active(table_mask, j)) { if (!first.emplace(key(0, j), j).second) dups++; }
    std::vector<uint64_t> cnt(n, 0);
    for (unsigned s = 0; s < nsets; s++) for (size_t i = 0; i < n; i++) if (is_active(lookup_mask, i)) {
        auto it = first.find(key(width * (1 + s), i));
        if (it != first.end()) cnt[it->second]++;
        else if (missing++ == 0) { first_set = s; first_row = i; }
    }
    REQUIRE(rep.missing == missing && rep.first_missing_set == first_set && rep.first_missing_row == first_row && rep.duplicate_table_rows == dups && rep.pad == 0);
    // a count c is c 2^64 mod p in Goldilocks; in the 252-bit field only zero / non-zero is compared here (tests/test_lookup_multiplicities.py compares the words)
    for (size_t j = 0; j < n; j++) {
        if (V == 1) REQUIRE(got[j] == cnt[j] * 0xFFFFFFFFull);
        else REQUIRE(((got[4 * j] | got[4 * j + 1] | got[4 * j + 2] | got[4 * j + 3]) != 0) == (cnt[j] != 0));
    }
    // refusals leave before anything is enqueued
    if (n) {
        REQUIRE(ms_lookup_multiplicities(ctx, field, n, dev.data(), nbase, width, &table, sets.data(), nsets, dev[0], d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
        ms_lookup_tuple bad = table;
        bad.cols[width - 1] = (int32_t)nbase;
        REQUIRE(ms_lookup_multiplicities(ctx, field, n, dev.data(), nbase, width, &bad, sets.data(), nsets, dev[m_col], d_report) == MS_ERR_INVALID);
    }
    const std::vector<ms_lookup_tuple> nine(MS_LOOKUP_MAX_SETS + 1, table);
    REQUIRE(ms_lookup_multiplicities(ctx, field, n, dev.data(), nbase, 0, &table, nine.data(), nsets, dev[m_col], d_report) == MS_ERR_INVALID);
    REQUIRE(ms_lookup_multiplicities(ctx, field, n, dev.data(), nbase, width, &table, nine.data(), MS_LOOKUP_MAX_SETS + 1, dev[m_col], d_report) == MS_ERR_UNSUPPORTED);
    for (void* p : dev) REQUIRE(ms_free(ctx, p) == MS_OK);
    REQUIRE(ms_free(ctx, d_report) == MS_OK);
    return 0;
}

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const size_t lengths[] = {0, 1, 2, 3, 7, 255, 256, 257, 1025};
    unsigned k = 0;
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (size_t n : lengths)
            for (unsigned width = 1; width <= MS_LOOKUP_MAX_WIDTH; width++, k++) {
                const unsigned nsets = k % 5 == 4 ? MS_LOOKUP_MAX_SETS : k % 4;           // 0 .. 3 and 8
                if (run(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, n, width, nsets, (int)(k % 3), (int)((k / 3) % 3))) return 1;
            }
    for (int checked = 0; checked < 2; checked++) {                    // and once in checked mode, which scans the named columns first
        REQUIRE(ms_ctx_set_checked(ctx, checked) == MS_OK);
        if (run(ctx, MS_GOLDILOCKS_FP, 1, 300, 2, 2, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO)) return 1;
    }
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("lookup sanitize ok\n");
    fflush(stdout);
    return 0;
}
