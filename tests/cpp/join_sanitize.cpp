// Host code and kernels of the row join (ministark_amd/csrc/ms_join.cpp, join_kernels.h, and lookup_kernels.h's build) under
// AddressSanitizer and UBSan, as a stand-alone CPU program: its own main, linked with the simulator build of the library's sources, where
// device memory is malloc'd memory and a slot, match entry or column index out of range is a heap overflow the sanitizer sees.  It runs
// ms_join_rows over table and probe lengths 0 .. 1025 crossed, widths 1 .. 4, both fields, masks on either side, 0 .. 8 sets, the
// self-join, and its refusals, compares every result with a std::map, and prints "join sanitize ok".  Not part of the suite (the build
// compiles every translation unit again); from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/join_sanitize.cpp -o join_sanitize -ldl && ./join_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>
#include "../../include/ministark_hip_join.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

static uint64_t lcg = 11;
static uint64_t next(uint64_t bound) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (lcg >> 33) % bound; }

struct Side {
    unsigned V; size_t rows; unsigned ncols;
    std::vector<std::vector<uint64_t>> host;
    std::vector<void*> dev;
    // small values v (the element is the words {v, 0, ..} with v in word c % V: below p in both fields, so canonical); the last column is the mask
    int fill(ms_ctx* ctx, unsigned V_, size_t rows_, unsigned ncols_, uint64_t values) {
        V = V_; rows = rows_; ncols = ncols_;
        host.assign(ncols, std::vector<uint64_t>(rows * V, 0));
        dev.assign(ncols, nullptr);
        for (unsigned c = 0; c < ncols; c++) {
            for (size_t i = 0; i < rows; i++) host[c][i * V + (c % V)] = next(c == ncols - 1 ? 2 : values);
            REQUIRE(ms_alloc(ctx, rows * V * 8 ? rows * V * 8 : 8, &dev[c]) == MS_OK);
            if (rows) REQUIRE(ms_upload(ctx, dev[c], host[c].data(), rows * V * 8) == MS_OK);
        }
        return 0;
    }
    bool active(int kind, size_t i) const {
        bool zero = true;
        for (unsigned l = 0; l < V; l++) zero = zero && host[ncols - 1][i * V + l] == 0;
        return kind == MS_EXT_ALWAYS || zero == (kind == MS_EXT_IF_ZERO);
    }
    std::vector<uint64_t> key(unsigned c0, unsigned width, size_t i) const {
        std::vector<uint64_t> k;
        for (unsigned c = 0; c < width; c++) for (unsigned l = 0; l < V; l++) k.push_back(host[c0 + c][i * V + l]);
        return k;
    }
    int release(ms_ctx* ctx) { for (void* p : dev) REQUIRE(ms_free(ctx, p) == MS_OK); return 0; }
};

// one call against a map; self: the probe side IS the table side (n == n_table)
static int run(ms_ctx* ctx, int field, unsigned V, size_t n_table, size_t n, unsigned width, unsigned nsets, int table_mask, int key_mask, bool self) {
    Side T, B;
    if (T.fill(ctx, V, n_table, width + 1, 3)) return 1;
    if (!self && B.fill(ctx, V, n, width * (nsets ? nsets : 1) + 1, 4)) return 1;
    const Side& P = self ? T : B;
    if (self) n = n_table;
    ms_lookup_tuple tkey = {{0, 0, 0, 0}, table_mask, (int32_t)(T.ncols - 1), 0, 0};
    std::vector<ms_lookup_tuple> sets(nsets, ms_lookup_tuple{{0, 0, 0, 0}, key_mask, (int32_t)(P.ncols - 1), 0, 0});
    for (unsigned c = 0; c < width; c++) { tkey.cols[c] = (int32_t)c; for (unsigned s = 0; s < nsets; s++) sets[s].cols[c] = (int32_t)(self ? c : width * s + c); }
    std::vector<void*> match(nsets ? nsets : 1, nullptr);
    for (auto& p : match) REQUIRE(ms_alloc(ctx, n * 4 ? n * 4 : 8, &p) == MS_OK);
    void* d_report = nullptr;
    REQUIRE(ms_alloc(ctx, sizeof(ms_join_report), &d_report) == MS_OK);
    REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, nsets ? sets.data() : nullptr, nsets,
                         nsets ? match.data() : nullptr, d_report) == MS_OK);
    ms_join_report rep;
    REQUIRE(ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
    std::map<std::vector<uint64_t>, size_t> first;
    uint64_t dups = 0, tact = 0, matched = 0, missing = 0, first_set = 0, first_row = 0;
    for (size_t j = 0; j < n_table; j++) if (T.active(table_mask, j)) { tact++; if (!first.emplace(T.key(0, width, j), j).second) dups++; }
    for (unsigned s = 0; s < nsets; s++) {
        std::vector<uint32_t> got(n), want(n, MS_JOIN_NONE);
        if (n) REQUIRE(ms_download(ctx, got.data(), match[s], n * 4) == MS_OK);
        for (size_t i = 0; i < n; i++) if (P.active(key_mask, i)) {
            auto it = first.find(P.key((unsigned)sets[s].cols[0], width, i));
            if (it != first.end()) { want[i] = (uint32_t)it->second; matched++; }
            else if (missing++ == 0) { first_set = s; first_row = i; }
        }
        REQUIRE(got == want);
        if (self && table_mask == MS_EXT_ALWAYS) for (size_t i = 0; i < n; i++) REQUIRE(want[i] == MS_JOIN_NONE || want[i] <= i);
    }
    REQUIRE(rep.matched == matched && rep.missing == missing && rep.first_missing_set == first_set && rep.first_missing_row == first_row && rep.pad == 0);
    REQUIRE(rep.duplicate_table_rows == dups && rep.table_active == tact);
    // refusals leave before anything is enqueued
    if (nsets && n && n_table) {
        std::vector<void*> bent = match;
        bent[nsets - 1] = T.dev[0];
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, sets.data(), nsets, bent.data(), d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
        bent[nsets - 1] = P.dev[(unsigned)sets[0].cols[0]];
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, sets.data(), nsets, bent.data(), d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, sets.data(), nsets, match.data(), match[0]) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
        bent = match;
        bent[0] = nullptr;
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, sets.data(), nsets, bent.data(), d_report) == MS_ERR_INVALID);
        ms_lookup_tuple bad = tkey;
        bad.cols[width - 1] = (int32_t)T.ncols;
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &bad, n, P.dev.data(), P.ncols, width, sets.data(), nsets, match.data(), d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "d_table"));
        std::vector<ms_lookup_tuple> bads = sets;
        bads[nsets - 1].mask = MS_EXT_IF_ZERO; bads[nsets - 1].mask_col = -1;
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, bads.data(), nsets, match.data(), d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "d_base"));
        bads = sets;
        bads[0].mask = 3;
        REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, bads.data(), nsets, match.data(), d_report) == MS_ERR_INVALID);
    }
    const std::vector<ms_lookup_tuple> nine(MS_JOIN_MAX_SETS + 1, sets.empty() ? tkey : sets[0]);
    const std::vector<void*> nine_out(MS_JOIN_MAX_SETS + 1, match[0]);
    REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, 0, nine.data(), nsets, match.data(), d_report) == MS_ERR_INVALID);
    REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, MS_JOIN_MAX_WIDTH + 1, nine.data(), nsets, match.data(), d_report) == MS_ERR_INVALID);
    REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, nine.data(), MS_JOIN_MAX_SETS + 1, nine_out.data(), d_report) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_join_rows(ctx, MS_GOLDILOCKS_FQ3, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, nine.data(), nsets, match.data(), d_report) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_join_rows(ctx, field, n_table, T.dev.data(), T.ncols, &tkey, n, P.dev.data(), P.ncols, width, nine.data(), nsets, match.data(), nullptr) == MS_ERR_INVALID);
    ms_join_report after;
    REQUIRE(ms_download(ctx, &after, d_report, sizeof after) == MS_OK && memcmp(&after, &rep, sizeof rep) == 0);      // no refusal wrote the report
    for (void* p : match) REQUIRE(ms_free(ctx, p) == MS_OK);
    REQUIRE(ms_free(ctx, d_report) == MS_OK);
    if (T.release(ctx) || (!self && B.release(ctx))) return 1;
    return 0;
}

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const size_t lengths[] = {0, 1, 2, 3, 7, 255, 256, 257, 1025};
    unsigned k = 0;
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (size_t n_table : lengths)
            for (size_t n : lengths)
                for (unsigned width = 1; width <= MS_JOIN_MAX_WIDTH; width++, k++) {
                    const unsigned nsets = k % 5 == 4 ? MS_JOIN_MAX_SETS : k % 4;         // 0 .. 3 and 8
                    if (run(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, n_table, n, width, nsets, (int)(k % 3), (int)((k / 3) % 3), false)) return 1;
                }
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})                 // d_table == d_base
        for (size_t n : lengths)
            for (int mask = 0; mask < 3; mask++)
                if (run(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, n, n, 1 + (unsigned)(n % 4), 2, mask, (mask + 1) % 3, true)) return 1;
    for (int checked = 0; checked < 2; checked++) {                    // and once in checked mode, which scans the named columns of both sides first
        REQUIRE(ms_ctx_set_checked(ctx, checked) == MS_OK);
        if (run(ctx, MS_GOLDILOCKS_FP, 1, 120, 300, 2, 2, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO, false)) return 1;
    }
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("join sanitize ok\n");
    fflush(stdout);
    return 0;
}
