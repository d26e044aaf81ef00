// Host code and kernels of the padded-table layer (ministark_amd/csrc/ms_gaps.cpp, gap_kernels.h) under AddressSanitizer and UBSan, as a
// stand-alone CPU program: its own main, linked with the simulator build of the library's sources, where device memory is malloc'd memory
// and an entry of start[], a staged slice, a source row or an output row out of range is a heap overflow the sanitizer sees.  It runs
// ms_gap_plan and ms_gap_fill over the lengths 0, 1, 2, T+1, 2T+1 (T = 1024, the positions of a tile), both fields, the three masks, 0 .. 3
// group columns, with and without a permutation (entries past the source included), output lengths below and above the table's, a run of
// inactive positions longer than the staged slice, and start[] arrays that no plan wrote; compares every Goldilocks start[] and counter
// column with a host loop on the canonical values; and tries the refusals; then prints "gap sanitize ok".  Not part of the suite (the build
// compiles every translation unit again); from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/gap_sanitize.cpp -o gap_sanitize -ldl && ./gap_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../include/ministark_hip_gaps.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

static uint64_t lcg = 17;
static uint64_t next(uint64_t bound) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (lcg >> 33) % bound; }

static const unsigned __int128 GLP = 0xFFFFFFFF00000001ull;
// the canonical value of a Goldilocks Montgomery word: w 2^-64 = w 2^128 (2^192 = 1 mod p), and back
static uint64_t gl_canon(uint64_t w) { return (uint64_t)((unsigned __int128)(w % (uint64_t)GLP) * 18446744065119617025ull % GLP); }
static uint64_t gl_mont(uint64_t v) { return (uint64_t)((unsigned __int128)(v % (uint64_t)GLP) * 0xFFFFFFFFull % GLP); }

// columns: 0 the counter (ascending along the positions), 1 a value, 2 .. 2 + ngroup the group columns, last the mask
static int run(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned ngroup, int mask, bool with_perm, size_t hole) {
    const unsigned nbase = 3 + ngroup, mask_col = nbase - 1;
    const size_t n_src = n + (with_perm ? 3 : 0);
    std::vector<std::vector<uint64_t>> host(nbase, std::vector<uint64_t>(n_src * V, 0));
    std::vector<uint32_t> perm(n);
    std::vector<size_t> where(n_src);
    std::iota(where.begin(), where.end(), (size_t)0);
    if (with_perm) for (size_t i = n_src; i > 1; i--) std::swap(where[i - 1], where[next(i)]);
    // a word below 2^32 in one limb is below p in both fields; over Goldilocks the word is the Montgomery form of some value, which
    // gl_canon recovers, so the counter is made to ascend in its CANONICAL value there
    uint64_t clock = 5, grp = 0;
    for (size_t j = 0; j < n; j++) {
        const size_t r = where[j];
        clock += 1 + (next(4) == 0 ? next(6) : 0);
        if (next(5) == 0) grp++;
        host[0][r * V] = V == 1 ? gl_mont(clock) : clock;           // over Fp252 the words are whatever they are: only bounds are checked
        host[1][r * V + (V - 1)] = next(1u << 31);
        for (unsigned g = 0; g < ngroup; g++) host[2 + g][r * V] = grp + g;
        host[mask_col][r * V] = hole && j >= 3 && j < 3 + hole ? (mask == MS_EXT_IF_ZERO ? 1 : 0) : next(3) ? 1 : 0;
        perm[j] = (uint32_t)r;
    }
    if (with_perm && n >= 3) { perm[1] = (uint32_t)n_src; perm[n - 1] = 0xFFFFFFFFu; }
    std::vector<void*> dev(nbase, nullptr);
    for (unsigned c = 0; c < nbase; c++) {
        REQUIRE(ms_alloc(ctx, n_src * V * 8 ? n_src * V * 8 : 8, &dev[c]) == MS_OK);
        if (n_src) REQUIRE(ms_upload(ctx, dev[c], host[c].data(), n_src * V * 8) == MS_OK);
    }
    void *d_perm = nullptr, *d_start = nullptr, *d_report = nullptr;
    REQUIRE(ms_alloc(ctx, n * 4 ? n * 4 : 8, &d_perm) == MS_OK);
    REQUIRE(ms_alloc(ctx, (n + 1) * 8, &d_start) == MS_OK);
    REQUIRE(ms_alloc(ctx, sizeof(ms_gap_report), &d_report) == MS_OK);
    if (n) REQUIRE(ms_upload(ctx, d_perm, perm.data(), n * 4) == MS_OK);
    ms_gap_spec spec = {{0, 0, 0}, (int32_t)ngroup, 0, mask, (int32_t)mask_col, 0};
    for (unsigned g = 0; g < ngroup; g++) spec.group[g] = (int32_t)(2 + g);
    const void* use_perm = with_perm ? d_perm : nullptr;
    REQUIRE(ms_gap_plan(ctx, field, n_src, dev.data(), nbase, &spec, use_perm, n, d_start, d_report) == MS_OK);
    std::vector<uint64_t> start(n + 1);
    ms_gap_report rep;
    REQUIRE(ms_download(ctx, start.data(), d_start, (n + 1) * 8) == MS_OK);
    REQUIRE(ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
    REQUIRE(start[0] == 0 && start[n] == rep.rows_out && std::is_sorted(start.begin(), start.end()));
    auto row = [&](size_t j) { return with_perm ? (size_t)perm[j] : j; };
    auto is_active = [&](size_t j) {
        if (row(j) >= n_src) return false;
        const bool zero = host[mask_col][row(j) * V] == 0;
        return mask == MS_EXT_ALWAYS || zero == (mask == MS_EXT_IF_ZERO);
    };
    uint64_t active = 0;
    for (size_t j = 0; j < n; j++) active += is_active(j);
    REQUIRE(rep.active == active && rep.rows_out >= active);
    if (V == 1) {                                                  // the loop of the header on canonical values
        uint64_t at = 0, gaps = 0, biggest = 0;
        for (size_t j = 0; j < n; j++) {
            REQUIRE(start[j] == at);
            if (!is_active(j)) continue;
            uint64_t gap = 0;
            bool same = j + 1 < n && is_active(j + 1);
            for (unsigned g = 0; same && g < ngroup; g++) same = host[2 + g][row(j)] == host[2 + g][row(j + 1)];
            if (same) gap = gl_canon(host[0][row(j + 1)]) - gl_canon(host[0][row(j)]) - 1;      // the clock ascends by construction
            at += 1 + gap; gaps += gap != 0; biggest = std::max(biggest, gap);
        }
        REQUIRE(start[n] == at && rep.gaps == gaps && rep.max_gap == biggest && rep.unordered == 0 && rep.saturated == 0 && rep.first_unordered == ~0ull);
    }
    // fill: shorter and longer than the table, every kind
    const ms_gap_column columns[4] = {{MS_GAP_COUNTER, 0}, {MS_GAP_COPY, 1}, {MS_GAP_ZERO, 1}, {MS_GAP_FLAG, 0}};
    // (over Fp252 the counters are whatever their words decode to, gaps of 2^32 among them: the head of such a table is enough)
    const size_t shown = (size_t)std::min<uint64_t>(rep.rows_out, 3 * n + 8);
    const size_t lengths[] = {shown / 2 + 1, shown + 1030};
    for (size_t n_out : lengths) {
        std::vector<void*> out(4, nullptr);
        for (auto& p : out) REQUIRE(ms_alloc(ctx, n_out * V * 8, &p) == MS_OK);
        REQUIRE(ms_gap_fill(ctx, field, n_src, dev.data(), nbase, use_perm, n, d_start, columns, out.data(), 4, n_out) == MS_OK);
        std::vector<uint64_t> got(n_out * V), flag(n_out * V);
        REQUIRE(ms_download(ctx, got.data(), out[0], n_out * V * 8) == MS_OK);
        REQUIRE(ms_download(ctx, flag.data(), out[3], n_out * V * 8) == MS_OK);
        if (V == 1 && rep.rows_out) {
            size_t s = 0;
            for (size_t j = 0; j < n_out; j++) {
                const uint64_t jj = std::min<uint64_t>(j, rep.rows_out - 1);
                while (s + 1 < n && start[s + 1] <= jj) s++;
                const uint64_t k = j - start[s];
                REQUIRE(gl_canon(got[j]) == (gl_canon(host[0][row(s)]) + k) % (uint64_t)GLP);
                REQUIRE(flag[j] == (k ? 0xFFFFFFFFull : 0ull));
            }
        }
        if (rep.rows_out == 0) for (size_t j = 0; j < n_out * V; j++) REQUIRE(got[j] == 0);
        // start[] that no plan wrote: the rows are not defined, the accesses stay in bounds
        if (n) {
            void* junk = nullptr;
            REQUIRE(ms_alloc(ctx, (n + 1) * 8, &junk) == MS_OK);
            std::vector<uint64_t> wild(n + 1);
            for (unsigned round = 0; round < 3; round++) {
                for (size_t j = 0; j <= n; j++) wild[j] = round == 0 ? n - j : round == 1 ? (next(1u << 31) << 33) | next(1u << 31) : ~0ull;
                REQUIRE(ms_upload(ctx, junk, wild.data(), (n + 1) * 8) == MS_OK);
                REQUIRE(ms_gap_fill(ctx, field, n_src, dev.data(), nbase, use_perm, n, junk, columns, out.data(), 4, n_out) == MS_OK);
            }
            REQUIRE(ms_free(ctx, junk) == MS_OK);
            // refusals leave before anything is enqueued
            std::vector<void*> bad = out;
            bad[1] = dev[1];
            REQUIRE(ms_gap_fill(ctx, field, n_src, dev.data(), nbase, use_perm, n, d_start, columns, bad.data(), 4, n_out) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
            bad = out; bad[2] = d_start;
            REQUIRE(ms_gap_fill(ctx, field, n_src, dev.data(), nbase, use_perm, n, d_start, columns, bad.data(), 4, n_out) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
            const ms_gap_column wrong[1] = {{MS_GAP_FLAG + 1, 0}};
            REQUIRE(ms_gap_fill(ctx, field, n_src, dev.data(), nbase, use_perm, n, d_start, wrong, out.data(), 1, n_out) == MS_ERR_INVALID);
        }
        for (void* p : out) REQUIRE(ms_free(ctx, p) == MS_OK);
    }
    if (n) REQUIRE(ms_gap_plan(ctx, field, n_src, dev.data(), nbase, &spec, use_perm, n, dev[0], d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    ms_gap_spec bad = spec;
    bad.counter = (int32_t)nbase;
    REQUIRE(ms_gap_plan(ctx, field, n_src, dev.data(), nbase, &bad, use_perm, n, d_start, d_report) == MS_ERR_INVALID);
    bad = spec; bad.ngroup = MS_GAP_MAX_GROUP + 1;
    REQUIRE(ms_gap_plan(ctx, field, n_src, dev.data(), nbase, &bad, use_perm, n, d_start, d_report) == MS_ERR_INVALID);
    for (void* p : dev) REQUIRE(ms_free(ctx, p) == MS_OK);
    REQUIRE(ms_free(ctx, d_perm) == MS_OK);
    REQUIRE(ms_free(ctx, d_start) == MS_OK);
    REQUIRE(ms_free(ctx, d_report) == MS_OK);
    return 0;
}

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const size_t T = 1024, lengths[] = {0, 1, 2, T + 1, 2 * T + 1};
    unsigned k = 0;
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (size_t n : lengths)
            for (unsigned twice = 0; twice < 2; twice++, k++)                              // 0 .. 3 group columns, the three masks and the permutation go round
                if (run(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, n, k % 4, (int)(k % 3), k % 2 == 1, 0)) return 1;
    // a run of inactive positions longer than the slice a fill workgroup stages (2048 entries)
    if (run(ctx, MS_GOLDILOCKS_FP, 1, 2300, 1, MS_EXT_IF_NONZERO, false, 2100)) return 1;
    if (run(ctx, MS_STARK252_FP, 4, 2300, 0, MS_EXT_IF_ZERO, true, 2100)) return 1;
    for (int checked = 0; checked < 2; checked++) {                    // and once in checked mode, which scans the named columns first
        REQUIRE(ms_ctx_set_checked(ctx, checked) == MS_OK);
        if (run(ctx, MS_GOLDILOCKS_FP, 1, 300, 2, MS_EXT_IF_NONZERO, true, 0)) return 1;
    }
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("gap sanitize ok\n");
    fflush(stdout);
    return 0;
}
