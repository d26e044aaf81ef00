// Host code and kernels of the range check (ministark_amd/csrc/ms_range.cpp and count_args.h; range_kernels.h on direct_count.h) under AddressSanitizer and UBSan, as a
// stand-alone CPU program: its own main, linked with the simulator build of the library's sources, where device memory is malloc'd memory
// and a limb column, a bin or a histogram word out of range is a heap (or global) overflow the sanitizer sees.  It runs ms_limb_decompose
// over lengths 0 .. 1025, every (bits, nlimbs) of tests/test_limb_decompose.py, both fields and the three masks, and
// ms_range_multiplicities over the same lengths, bits 1 .. 17, 0 .. 64 sets and every counting form (MS_RANGE_FORM unset, plain, lds),
// with a run long enough for the packed counters to flush; compares every word with a plain loop that extracts bit by bit, checks the
// refusals, and prints "range sanitize ok".  Not part of the suite (the build compiles every translation unit again); from the
// repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/range_sanitize.cpp -o range_sanitize -ldl && ./range_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/ministark_hip_range.h"
#include "../../ministark_amd/csrc/gl.h"
#include "../../ministark_amd/csrc/fp252.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

static uint64_t lcg = 29;
static uint64_t next64() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; uint64_t hi = lcg >> 32; lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return hi << 32 | lcg >> 32; }

struct Value { uint64_t w[4]; };                                     // a canonical integer, least significant word first (w[1..3] = 0 over Fp)

static Value draw(unsigned V, unsigned small_bits) {
    Value v = {{0, 0, 0, 0}};
    const unsigned kind = (unsigned)(next64() % 4);
    if (kind == 0) { v.w[0] = small_bits >= 64 ? next64() : next64() & ((1ull << small_bits) - 1); }               // fits `small_bits` bits
    else if (kind == 1 && V == 4) { v.w[3] = next64() & ((1ull << 59) - 1); }                                     // the top word alone
    else { for (unsigned l = 0; l < V; l++) v.w[l] = next64(); if (V == 4) v.w[3] &= (1ull << 59) - 1; }
    if (V == 1) v.w[0] %= gl::P;
    return v;
}
static void to_words(unsigned V, const Value& v, uint64_t* out) {
    if (V == 1) { out[0] = gl::to_mont(v.w[0]); return; }
    const f252::E m = f252::to_mont(f252::E{{v.w[0], v.w[1], v.w[2], v.w[3]}});
    memcpy(out, m.l, 32);
}
static unsigned bit(const Value& v, unsigned k) { return k < 256 ? (unsigned)(v.w[k >> 6] >> (k & 63)) & 1u : 0u; }
static bool is_zero(const Value& v) { return (v.w[0] | v.w[1] | v.w[2] | v.w[3]) == 0; }

struct Trace {
    unsigned V; size_t n;
    std::vector<std::vector<Value>> host;
    std::vector<void*> dev;
    int make(ms_ctx* ctx, unsigned V_, size_t n_, unsigned ncols, unsigned nfilled, unsigned small_bits) {        // columns from nfilled on hold all ones
        V = V_; n = n_;
        host.assign(ncols, std::vector<Value>(n, Value{{0, 0, 0, 0}}));
        dev.assign(ncols, nullptr);
        for (unsigned c = 0; c < ncols; c++) {
            std::vector<uint64_t> w(n * V + 1, ~0ull);
            if (c < nfilled) for (size_t i = 0; i < n; i++) {
                host[c][i] = c + 1 == nfilled ? Value{{next64() % 3 ? next64() % gl::P : 0, 0, 0, 0}} : draw(V, small_bits);          // the last filled column is the mask
                to_words(V, host[c][i], &w[i * V]);
            }
            REQUIRE(ms_alloc(ctx, n * V * 8 ? n * V * 8 : 8, &dev[c]) == MS_OK);                                     // exactly the column: one word more is an overflow
            if (n) REQUIRE(ms_upload(ctx, dev[c], w.data(), n * V * 8) == MS_OK);
        }
        return 0;
    }
    bool active(int kind, unsigned mask_col, size_t i) const { return kind == MS_EXT_ALWAYS || is_zero(host[mask_col][i]) == (kind == MS_EXT_IF_ZERO); }
    int release(ms_ctx* ctx) { for (void* p : dev) REQUIRE(ms_free(ctx, p) == MS_OK); return 0; }
};

static int run_limbs(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned bits, unsigned nlimbs, int mask) {
    // columns: 0, 1 sources, 2 mask, then two specs' destinations
    Trace T;
    if (T.make(ctx, V, n, 3 + 2 * nlimbs, 3, bits * nlimbs)) return 1;
    const ms_limb_spec specs[2] = {{0, 3, (int32_t)nlimbs, (int32_t)bits, mask, 2, 0, 0}, {1, (int32_t)(3 + nlimbs), (int32_t)nlimbs, (int32_t)bits, (mask + 1) % 3, 2, 0, 0}};
    void* d_report = nullptr;
    REQUIRE(ms_alloc(ctx, sizeof(ms_limb_report), &d_report) == MS_OK);
    REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), specs, 2, d_report) == MS_OK);
    ms_limb_report rep;
    REQUIRE(ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
    uint64_t overflow = 0, active = 0, first_spec = 0, first_row = 0;
    for (unsigned k = 0; k < 2; k++) {
        for (unsigned j = 0; j < nlimbs; j++) {
            std::vector<uint64_t> got(n * V), want(n * V, 0);
            if (n) REQUIRE(ms_download(ctx, got.data(), T.dev[specs[k].dst0 + j], n * V * 8) == MS_OK);
            for (size_t i = 0; i < n; i++) if (T.active(specs[k].mask, 2, i)) {
                Value limb = {{0, 0, 0, 0}};
                for (unsigned b = 0; b < bits; b++) limb.w[0] |= (uint64_t)bit(T.host[k][i], j * bits + b) << b;
                to_words(V, limb, &want[i * V]);
            }
            REQUIRE(got == want);
        }
        for (size_t i = 0; i < n; i++) if (T.active(specs[k].mask, 2, i)) {
            active++;
            bool over = false;
            for (unsigned b = bits * nlimbs; b < 256; b++) over = over || bit(T.host[k][i], b);
            if (over && overflow++ == 0) { first_spec = k; first_row = i; }
        }
    }
    REQUIRE(rep.overflow == overflow && rep.first_overflow_spec == first_spec && rep.first_overflow_row == first_row && rep.active == active && rep.pad == 0);
    // refusals leave before anything is enqueued
    ms_limb_spec bad[2] = {specs[0], specs[1]};
    bad[1].dst0 = 3 + (int32_t)nlimbs + 1;                                       // the last limb column would be past the table
    REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), bad, 2, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "out of range"));
    bad[1] = specs[1]; bad[1].dst0 = 3;
    REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), bad, 2, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    bad[1] = specs[1]; bad[1].dst0 = 2;
    REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), bad, 2, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    bad[1] = specs[1]; bad[1].nlimbs = (int32_t)(64 * V / bits + 1);
    REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), bad, 2, d_report) == MS_ERR_INVALID);
    bad[1] = specs[1]; bad[1].bits = 33;
    REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), bad, 2, d_report) == MS_ERR_INVALID);
    if (n * V * 8 >= sizeof(ms_limb_report)) REQUIRE(ms_limb_decompose(ctx, field, n, T.dev.data(), (unsigned)T.dev.size(), specs, 2, T.dev[3]) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    REQUIRE(ms_limb_decompose(ctx, MS_GOLDILOCKS_FQ3, n, T.dev.data(), (unsigned)T.dev.size(), specs, 2, d_report) == MS_ERR_UNSUPPORTED);
    ms_limb_report after;
    REQUIRE(ms_download(ctx, &after, d_report, sizeof after) == MS_OK && memcmp(&after, &rep, sizeof rep) == 0);      // no refusal wrote the report
    REQUIRE(ms_free(ctx, d_report) == MS_OK);
    return T.release(ctx);
}

static int run_counts(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned bits, unsigned nsets, int mask, size_t tail, bool one_value) {
    // columns: 0, 1 looked up, 2 mask
    Trace T;
    if (T.make(ctx, V, n, 3, 3, bits)) return 1;
    if (one_value) for (size_t i = 0; i < n; i++) T.host[0][i] = T.host[1][i] = Value{{(1ull << bits) - 1, 0, 0, 0}};
    if (one_value) for (unsigned c = 0; c < 2; c++) {
        std::vector<uint64_t> w(n * V);
        for (size_t i = 0; i < n; i++) to_words(V, T.host[c][i], &w[i * V]);
        if (n) REQUIRE(ms_upload(ctx, T.dev[c], w.data(), n * V * 8) == MS_OK);
    }
    std::vector<ms_range_set> sets(nsets);
    for (unsigned s = 0; s < nsets; s++) sets[s] = ms_range_set{(int32_t)(s % 2), (int32_t)((mask + s) % 3), 2, 0};
    const size_t bins = (size_t)1 << bits, n_m = bins + tail;
    void *d_m = nullptr, *d_report = nullptr;
    REQUIRE(ms_alloc(ctx, n_m * V * 8, &d_m) == MS_OK && ms_alloc(ctx, sizeof(ms_lookup_report), &d_report) == MS_OK);
    std::vector<uint64_t> cnt(bins, 0);
    uint64_t missing = 0, first_set = 0, first_row = 0;
    for (unsigned s = 0; s < nsets; s++)
        for (size_t i = 0; i < n; i++) if (T.active(sets[s].mask, 2, i)) {
            const Value& v = T.host[sets[s].col][i];
            if ((v.w[1] | v.w[2] | v.w[3]) == 0 && v.w[0] < bins) cnt[v.w[0]]++;
            else if (missing++ == 0) { first_set = s; first_row = i; }
        }
    std::vector<uint64_t> want(n_m * V, 0);
    for (size_t j = 0; j < bins; j++) to_words(V, Value{{cnt[j], 0, 0, 0}}, &want[j * V]);
    ms_lookup_report rep;
    for (const char* form : {"", "plain", "lds"}) {
        if (*form) setenv("MS_RANGE_FORM", form, 1); else unsetenv("MS_RANGE_FORM");
        std::vector<uint64_t> got(n_m * V, ~0ull);
        REQUIRE(ms_upload(ctx, d_m, got.data(), n_m * V * 8) == MS_OK);
        REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, bits, nsets ? sets.data() : nullptr, nsets, n_m, d_m, d_report) == MS_OK);
        REQUIRE(ms_download(ctx, got.data(), d_m, n_m * V * 8) == MS_OK && ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
        REQUIRE(got == want);
        REQUIRE(rep.missing == missing && rep.first_missing_set == first_set && rep.first_missing_row == first_row && rep.pad == 0 && rep.duplicate_table_rows == 0);
    }
    unsetenv("MS_RANGE_FORM");
    // refusals leave before anything is enqueued
    const std::vector<ms_range_set> many(MS_RANGE_MAX_SETS + 1, ms_range_set{0, 0, 0, 0});
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, bits, many.data(), MS_RANGE_MAX_SETS + 1, n_m, d_m, d_report) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, bits, many.data(), 1, bins - 1, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, 0, many.data(), 1, n_m, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, 25, many.data(), 1, (size_t)1 << 25, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_range_multiplicities(ctx, field, (size_t)1 << 26, T.dev.data(), 3, bits, many.data(), MS_RANGE_MAX_SETS, n_m, d_m, d_report) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_range_multiplicities(ctx, MS_GOLDILOCKS_FQ3, n, T.dev.data(), 3, bits, many.data(), 1, n_m, d_m, d_report) == MS_ERR_UNSUPPORTED);
    ms_range_set bad = {3, 0, 0, 0};
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, bits, &bad, 1, n_m, d_m, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "out of range"));
    bad = ms_range_set{0, 3, 0, 0};
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, bits, &bad, 1, n_m, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_range_multiplicities(ctx, field, n, T.dev.data(), 3, bits, many.data(), 1, n_m, d_m, d_m) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    ms_lookup_report after;
    REQUIRE(ms_download(ctx, &after, d_report, sizeof after) == MS_OK && memcmp(&after, &rep, sizeof rep) == 0);      // no refusal wrote the report
    REQUIRE(ms_free(ctx, d_m) == MS_OK && ms_free(ctx, d_report) == MS_OK);
    return T.release(ctx);
}

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const size_t lengths[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025};
    const unsigned fp_shapes[][2] = {{1, 64}, {16, 4}, {32, 2}, {7, 9}, {12, 5}, {20, 3}, {24, 2}}, fp252_shapes[][2] = {{32, 8}, {28, 9}, {1, 252}, {16, 16}, {28, 8}, {31, 3}};
    unsigned k = 0;
    for (size_t n : lengths) {
        for (auto& s : fp_shapes) if (run_limbs(ctx, MS_GOLDILOCKS_FP, 1, n, s[0], s[1], (int)(k++ % 3))) return 1;
        for (auto& s : fp252_shapes) if (run_limbs(ctx, MS_STARK252_FP, 4, n, s[0], s[1], (int)(k++ % 3))) return 1;
    }
    const unsigned table_bits[] = {1, 5, 8, 12, 13, 15, 16, 17};
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (size_t n : lengths)
            for (unsigned bits : table_bits) {
                const unsigned nsets = k % 7 == 6 ? MS_RANGE_MAX_SETS : k % 4;          // 0 .. 3 and 64
                if (run_counts(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, n, bits, nsets, (int)(k % 3), k % 5, false)) return 1;
                k++;
            }
    // 70 000 rows on the last bin, two sets: the packed counters of bits = 16 flush in the middle of the run; and the largest 32-bit table
    if (run_counts(ctx, MS_GOLDILOCKS_FP, 1, 70000, 16, 2, MS_EXT_ALWAYS, 3, true)) return 1;
    if (run_counts(ctx, MS_GOLDILOCKS_FP, 1, 70000, 15, 2, MS_EXT_ALWAYS, 0, true)) return 1;
    for (int checked = 0; checked < 2; checked++) {                    // and once in checked mode, which scans the named columns first
        REQUIRE(ms_ctx_set_checked(ctx, checked) == MS_OK);
        if (run_limbs(ctx, MS_STARK252_FP, 4, 300, 28, 9, MS_EXT_IF_NONZERO)) return 1;
        if (run_counts(ctx, MS_STARK252_FP, 4, 300, 9, 3, MS_EXT_IF_ZERO, 2, false)) return 1;
    }
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("range sanitize ok\n");
    fflush(stdout);
    return 0;
}
