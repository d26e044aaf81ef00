// Host code and kernels of the bitwise-operation columns (ministark_amd/csrc/ms_bitwise.cpp and count_args.h; bitwise_kernels.h on direct_count.h) under AddressSanitizer and
// UBSan, as a stand-alone CPU program: its own main, linked with the simulator build of the library's sources, where device memory is
// malloc'd memory and a result column, a bin or a histogram word out of range is a heap (or global) overflow the sanitizer sees.  It runs
// ms_bitwise_columns over lengths 0 .. 1025, widths from 1 to WMAX, the three ops, both fields and the three masks; ms_bitwise_table for
// every bits 1 .. 9 it then counts against; and ms_bitwise_multiplicities over the same lengths, bits 1 .. 9, one to three ops, 0 .. 64
// sets and every counting form (MS_BITWISE_FORM unset, plain, lds), with a run long enough for the packed counters to flush more than once;
// compares every word with a plain loop that works bit by bit, checks the refusals, and prints "bitwise sanitize ok".  Not part of the
// suite (the build compiles every translation unit again); from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/bitwise_sanitize.cpp -o bitwise_sanitize -ldl && ./bitwise_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/ministark_hip_bitwise.h"
#include "../../ministark_amd/csrc/gl.h"
#include "../../ministark_amd/csrc/fp252.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

static uint64_t lcg = 31;
static uint64_t next64() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; uint64_t hi = lcg >> 32; lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return hi << 32 | lcg >> 32; }

struct Value { uint64_t w[4]; };                                     // a canonical integer, least significant word first (w[1..3] = 0 over Fp)

static unsigned bit(const Value& v, unsigned k) { return k < 256 ? (unsigned)(v.w[k >> 6] >> (k & 63)) & 1u : 0u; }
static void set_bit(Value& v, unsigned k, unsigned b) { v.w[k >> 6] |= (uint64_t)b << (k & 63); }
static bool is_zero(const Value& v) { return (v.w[0] | v.w[1] | v.w[2] | v.w[3]) == 0; }
static bool same(const Value& a, const Value& b) { return !memcmp(a.w, b.w, 32); }
static bool fits(const Value& v, unsigned total) { for (unsigned k = total; k < 256; k++) if (bit(v, k)) return false; return true; }
static unsigned op_bit(int op, unsigned x, unsigned y) { return op == MS_BIT_AND ? x & y : op == MS_BIT_OR ? x | y : x ^ y; }
static Value combine(int op, const Value& a, const Value& b, unsigned width) {          // bit by bit, the low `width` bits
    Value r = {{0, 0, 0, 0}};
    for (unsigned k = 0; k < width && k < 256; k++) set_bit(r, k, op_bit(op, bit(a, k), bit(b, k)));
    return r;
}
static unsigned limb(const Value& v, unsigned j, unsigned bits) { unsigned x = 0; for (unsigned b = 0; b < bits; b++) x |= bit(v, j * bits + b) << b; return x; }

// mostly values of `small_bits` bits; some that do not fit: one bit higher, the top word alone (Fp252), anything canonical
static Value draw(unsigned V, unsigned small_bits) {
    Value v = {{0, 0, 0, 0}};
    const unsigned kind = (unsigned)(next64() % 8);
    if (kind == 0 && V == 4) v.w[3] = next64() & ((1ull << 59) - 1);
    else if (kind == 1) { for (unsigned l = 0; l < V; l++) v.w[l] = next64(); if (V == 4) v.w[3] &= (1ull << 59) - 1; }
    else {
        for (unsigned k = 0; k < small_bits; k++) set_bit(v, k, (unsigned)(next64() >> 63));
        if (kind == 2 && small_bits < (V == 1 ? 63u : 251u)) set_bit(v, small_bits, 1);
    }
    if (V == 1) v.w[0] %= gl::P;
    return v;
}
static void to_words(unsigned V, const Value& v, uint64_t* out) {
    if (V == 1) { out[0] = gl::to_mont(v.w[0]); return; }
    const f252::E m = f252::to_mont(f252::E{{v.w[0], v.w[1], v.w[2], v.w[3]}});
    memcpy(out, m.l, 32);
}

struct Trace {
    unsigned V; size_t n;
    std::vector<std::vector<Value>> host;
    std::vector<void*> dev;
    int upload(ms_ctx* ctx, unsigned c) {
        std::vector<uint64_t> w(n * V + 1);
        for (size_t i = 0; i < n; i++) to_words(V, host[c][i], &w[i * V]);
        if (n) REQUIRE(ms_upload(ctx, dev[c], w.data(), n * V * 8) == MS_OK);
        return 0;
    }
    int make(ms_ctx* ctx, unsigned V_, size_t n_, unsigned ncols, unsigned nfilled, unsigned small_bits) {        // columns from nfilled on hold all ones
        V = V_; n = n_;
        host.assign(ncols, std::vector<Value>(n, Value{{0, 0, 0, 0}}));
        dev.assign(ncols, nullptr);
        for (unsigned c = 0; c < ncols; c++) {
            REQUIRE(ms_alloc(ctx, n * V * 8 ? n * V * 8 : 8, &dev[c]) == MS_OK);                                     // exactly the column: one word more is an overflow
            if (c < nfilled) {
                for (size_t i = 0; i < n; i++) host[c][i] = c + 1 == nfilled ? Value{{next64() % 3 ? next64() % gl::P : 0, 0, 0, 0}} : draw(V, small_bits);   // the last filled column is the mask
                if (upload(ctx, c)) return 1;
            } else {
                std::vector<uint64_t> w(n * V + 1, ~0ull);
                if (n) REQUIRE(ms_upload(ctx, dev[c], w.data(), n * V * 8) == MS_OK);
            }
        }
        return 0;
    }
    bool active(int kind, unsigned mask_col, size_t i) const { return kind == MS_EXT_ALWAYS || is_zero(host[mask_col][i]) == (kind == MS_EXT_IF_ZERO); }
    int release(ms_ctx* ctx) { for (void* p : dev) REQUIRE(ms_free(ctx, p) == MS_OK); return 0; }
};

static int run_columns(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned width, int mask) {
    // columns: 0, 1 operands, 2 mask, 3 .. 5 the destinations of AND, OR, XOR; the XOR is of column 1 with itself
    Trace T;
    if (T.make(ctx, V, n, 6, 3, width)) return 1;
    const ms_bitwise_spec specs[3] = {{MS_BIT_AND, 0, 1, 3, (int32_t)width, mask, 2, 0}, {MS_BIT_OR, 1, 0, 4, (int32_t)width, (mask + 1) % 3, 2, 0},
                                      {MS_BIT_XOR, 1, 1, 5, (int32_t)width, (mask + 2) % 3, 2, 0}};
    void* d_report = nullptr;
    REQUIRE(ms_alloc(ctx, sizeof(ms_limb_report), &d_report) == MS_OK);
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, specs, 3, d_report) == MS_OK);
    ms_limb_report rep;
    REQUIRE(ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
    uint64_t overflow = 0, active = 0, first_spec = 0, first_row = 0;
    for (unsigned k = 0; k < 3; k++) {
        std::vector<uint64_t> got(n * V), want(n * V, 0);
        if (n) REQUIRE(ms_download(ctx, got.data(), T.dev[specs[k].dst], n * V * 8) == MS_OK);
        for (size_t i = 0; i < n; i++) if (T.active(specs[k].mask, 2, i)) {
            const Value &a = T.host[specs[k].a][i], &b = T.host[specs[k].b][i];
            to_words(V, combine(specs[k].op, a, b, width), &want[i * V]);
            active++;
            if ((!fits(a, width) || !fits(b, width)) && overflow++ == 0) { first_spec = k; first_row = i; }
        }
        REQUIRE(got == want);
    }
    REQUIRE(rep.overflow == overflow && rep.first_overflow_spec == first_spec && rep.first_overflow_row == first_row && rep.active == active && rep.pad == 0);
    // refusals leave before anything is enqueued
    ms_bitwise_spec bad[3] = {specs[0], specs[1], specs[2]};
    bad[1].dst = 6;
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, bad, 3, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "out of range"));
    bad[1] = specs[1]; bad[1].dst = 3;
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, bad, 3, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    bad[1] = specs[1]; bad[1].dst = 2;
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, bad, 3, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    bad[1] = specs[1]; bad[1].width = V == 1 ? 64 : 252;
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, bad, 3, d_report) == MS_ERR_INVALID);
    bad[1] = specs[1]; bad[1].width = 0;
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, bad, 3, d_report) == MS_ERR_INVALID);
    bad[1] = specs[1]; bad[1].op = 3;
    REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, bad, 3, d_report) == MS_ERR_INVALID);
    if (n * V * 8 >= sizeof(ms_limb_report)) REQUIRE(ms_bitwise_columns(ctx, field, n, T.dev.data(), 6, specs, 3, T.dev[3]) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    REQUIRE(ms_bitwise_columns(ctx, MS_GOLDILOCKS_FQ3, n, T.dev.data(), 6, specs, 3, d_report) == MS_ERR_UNSUPPORTED);
    ms_limb_report after;
    REQUIRE(ms_download(ctx, &after, d_report, sizeof after) == MS_OK && memcmp(&after, &rep, sizeof rep) == 0);      // no refusal wrote the report
    REQUIRE(ms_free(ctx, d_report) == MS_OK);
    return T.release(ctx);
}

static int run_table(ms_ctx* ctx, int field, unsigned V, unsigned bits, const int32_t* ops, unsigned nops, size_t tail, bool with_op) {
    const size_t T = (size_t)nops << (2 * bits), n_t = T + tail;
    void* d[4];
    for (auto& p : d) REQUIRE(ms_alloc(ctx, n_t * V * 8, &p) == MS_OK);
    REQUIRE(ms_bitwise_table(ctx, field, bits, ops, nops, n_t, with_op ? d[0] : nullptr, d[1], d[2], d[3]) == MS_OK);
    std::vector<uint64_t> got(n_t * V), want(n_t * V);
    for (unsigned c = with_op ? 0 : 1; c < 4; c++) {
        for (size_t j = 0; j < n_t; j++) {
            const size_t r = j < T ? j : T - 1;
            const unsigned s = (unsigned)(r >> (2 * bits)), x = (unsigned)(r >> bits) & ((1u << bits) - 1), y = (unsigned)r & ((1u << bits) - 1);
            unsigned z = 0;
            for (unsigned b = 0; b < bits; b++) z |= op_bit(ops[s], (x >> b) & 1, (y >> b) & 1) << b;
            to_words(V, Value{{c == 0 ? (uint64_t)ops[s] : c == 1 ? x : c == 2 ? y : z, 0, 0, 0}}, &want[j * V]);
        }
        REQUIRE(ms_download(ctx, got.data(), d[c], n_t * V * 8) == MS_OK && got == want);
    }
    REQUIRE(ms_bitwise_table(ctx, field, bits, ops, nops, T - 1, d[0], d[1], d[2], d[3]) == MS_ERR_INVALID);
    REQUIRE(ms_bitwise_table(ctx, field, bits, ops, nops, n_t, d[0], d[1], d[1], d[3]) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    REQUIRE(ms_bitwise_table(ctx, field, 13, ops, nops, n_t, d[0], d[1], d[2], d[3]) == MS_ERR_INVALID);
    REQUIRE(ms_bitwise_table(ctx, MS_GOLDILOCKS_FQ3, bits, ops, nops, n_t, d[0], d[1], d[2], d[3]) == MS_ERR_UNSUPPORTED);
    for (auto& p : d) REQUIRE(ms_free(ctx, p) == MS_OK);
    return 0;
}

// shape: 0 drawn operands, 1 every operand zero, 2 a zero and b alternating between all-zero and all-one limbs (the two bins of one word)
static int run_counts(ms_ctx* ctx, int field, unsigned V, size_t n, unsigned bits, unsigned nops, unsigned nlimbs, unsigned nsets, int mask, size_t tail, int shape) {
    // columns: 0, 1 operands, 2 .. 4 the AND, OR, XOR of both, a few of them wrong, 5 mask
    static const int32_t all_ops[3] = {MS_BIT_XOR, MS_BIT_AND, MS_BIT_OR};
    const int32_t* ops = all_ops;
    Trace T;
    if (T.make(ctx, V, n, 6, 6, nlimbs * bits)) return 1;
    for (size_t i = 0; i < n && shape; i++) {
        T.host[0][i] = T.host[1][i] = Value{{0, 0, 0, 0}};
        if (shape == 2 && (i & 1)) for (unsigned j = 0; j < nlimbs; j++) set_bit(T.host[1][i], j * bits, 1);
    }
    for (unsigned c = 2; c < 5; c++) {
        for (size_t i = 0; i < n; i++) {
            T.host[c][i] = combine((int)c - 2, T.host[0][i], T.host[1][i], 256);
            if (shape == 0 && next64() % 16 == 0) T.host[c][i].w[0] ^= 1ull << (next64() % (nlimbs * bits < 64 ? nlimbs * bits : 64));   // a wrong result, still canonical
        }
    }
    if (shape) { static const Value zero = {{0, 0, 0, 0}}; for (size_t i = 0; i < n; i++) T.host[5][i] = zero; }
    for (unsigned c = 0; c < 6; c++) if (T.upload(ctx, c)) return 1;
    std::vector<ms_bitwise_set> sets(nsets);
    for (unsigned s = 0; s < nsets; s++) {
        const int32_t op = ops[s % nops];
        sets[s] = ms_bitwise_set{op, (int32_t)(s % 2), (int32_t)(1 - s % 2), s % 3 == 2 ? -1 : 2 + op, (int32_t)(shape ? nlimbs : 1 + (s + nlimbs - 1) % nlimbs),
                                 shape ? MS_EXT_ALWAYS : (int32_t)((mask + s) % 3), 5, 0};
    }
    const size_t bins = (size_t)1 << (2 * bits), Trows = nops * bins, n_m = Trows + tail;
    void *d_m = nullptr, *d_report = nullptr;
    REQUIRE(ms_alloc(ctx, n_m * V * 8, &d_m) == MS_OK && ms_alloc(ctx, sizeof(ms_lookup_report), &d_report) == MS_OK);
    std::vector<uint64_t> cnt(Trows, 0);
    uint64_t missing = 0, first_set = 0, first_row = 0;
    for (unsigned s = 0; s < nsets; s++)
        for (size_t i = 0; i < n; i++) if (T.active(sets[s].mask, 5, i)) {
            const Value &a = T.host[sets[s].a][i], &b = T.host[sets[s].b][i];
            const unsigned total = (unsigned)sets[s].nlimbs * bits;
            const bool ok = fits(a, total) && fits(b, total) && (sets[s].c < 0 || same(T.host[sets[s].c][i], combine(sets[s].op, a, b, 256)));
            if (!ok) { if (missing++ == 0) { first_set = s; first_row = i; } continue; }
            for (unsigned j = 0; j < (unsigned)sets[s].nlimbs; j++) cnt[(s % nops) * bins + ((size_t)limb(a, j, bits) << bits) + limb(b, j, bits)]++;
        }
    std::vector<uint64_t> want(n_m * V, 0);
    for (size_t j = 0; j < Trows; j++) if (cnt[j]) to_words(V, Value{{cnt[j], 0, 0, 0}}, &want[j * V]);
    ms_lookup_report rep;
    for (const char* form : {"", "plain", "lds"}) {
        if (*form) setenv("MS_BITWISE_FORM", form, 1); else unsetenv("MS_BITWISE_FORM");
        std::vector<uint64_t> got(n_m * V, ~0ull);
        REQUIRE(ms_upload(ctx, d_m, got.data(), n_m * V * 8) == MS_OK);
        REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, nsets ? sets.data() : nullptr, nsets, n_m, d_m, d_report) == MS_OK);
        REQUIRE(ms_download(ctx, got.data(), d_m, n_m * V * 8) == MS_OK && ms_download(ctx, &rep, d_report, sizeof rep) == MS_OK);
        REQUIRE(got == want);
        REQUIRE(rep.missing == missing && rep.first_missing_set == first_set && rep.first_missing_row == first_row && rep.pad == 0 && rep.duplicate_table_rows == 0);
    }
    unsetenv("MS_BITWISE_FORM");
    // refusals leave before anything is enqueued
    const ms_bitwise_set one = {ops[0], 0, 1, -1, 1, 0, 0, 0};
    const std::vector<ms_bitwise_set> many(MS_BITWISE_MAX_SETS + 1, one);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, many.data(), MS_BITWISE_MAX_SETS + 1, n_m, d_m, d_report) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, many.data(), 1, Trows - 1, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, 0, ops, nops, many.data(), 1, n_m, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, 13, ops, nops, many.data(), 1, n_m, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, (size_t)1 << 26, T.dev.data(), 6, bits, ops, nops, many.data(), MS_BITWISE_MAX_SETS, n_m, d_m, d_report) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_bitwise_multiplicities(ctx, MS_GOLDILOCKS_FQ3, n, T.dev.data(), 6, bits, ops, nops, many.data(), 1, n_m, d_m, d_report) == MS_ERR_UNSUPPORTED);
    ms_bitwise_set bad = one;
    bad.b = 6;
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, &bad, 1, n_m, d_m, d_report) == MS_ERR_INVALID && strstr(ms_last_error(), "out of range"));
    bad = one; bad.nlimbs = (int32_t)((V == 1 ? 63 : 251) / bits + 1);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, &bad, 1, n_m, d_m, d_report) == MS_ERR_INVALID);
    bad = one; bad.op = nops < 3 ? ops[2] : 7;
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, &bad, 1, n_m, d_m, d_report) == MS_ERR_INVALID);
    REQUIRE(ms_bitwise_multiplicities(ctx, field, n, T.dev.data(), 6, bits, ops, nops, many.data(), 1, n_m, d_m, d_m) == MS_ERR_INVALID && strstr(ms_last_error(), "overlap"));
    ms_lookup_report after;
    REQUIRE(ms_download(ctx, &after, d_report, sizeof after) == MS_OK && memcmp(&after, &rep, sizeof rep) == 0);      // no refusal wrote the report
    REQUIRE(ms_free(ctx, d_m) == MS_OK && ms_free(ctx, d_report) == MS_OK);
    return T.release(ctx);
}

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const size_t lengths[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025};
    const unsigned fp_widths[] = {1, 8, 31, 32, 33, 63}, fp252_widths[] = {1, 63, 64, 65, 128, 192, 193, 251};
    unsigned k = 0;
    for (size_t n : lengths) {
        for (unsigned w : fp_widths) if (run_columns(ctx, MS_GOLDILOCKS_FP, 1, n, w, (int)(k++ % 3))) return 1;
        for (unsigned w : fp252_widths) if (run_columns(ctx, MS_STARK252_FP, 4, n, w, (int)(k++ % 3))) return 1;
    }
    static const int32_t table_ops[3] = {MS_BIT_OR, MS_BIT_XOR, MS_BIT_AND};
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (unsigned bits = 1; bits <= 9; bits++, k++)
            if (run_table(ctx, field, field == MS_GOLDILOCKS_FP ? 1 : 4, bits, table_ops + k % 2, 1 + k % 2, k % 5, k % 3 != 0)) return 1;
    for (int field : {MS_GOLDILOCKS_FP, MS_STARK252_FP})
        for (size_t n : lengths)
            for (unsigned bits = 1; bits <= 9; bits++) {
                const unsigned V = field == MS_GOLDILOCKS_FP ? 1 : 4, wmax = V == 1 ? 63 : 251;
                const unsigned nsets = k % 7 == 6 ? MS_BITWISE_MAX_SETS : k % 4;       // 0 .. 3 and 64
                const unsigned most = wmax / bits, nlimbs = k % 5 == 0 ? most : 1 + k % (most < 9 ? most : 9);       // the widest operand, limbs across word boundaries
                if (run_counts(ctx, field, V, n, bits, 1 + k % 3, nlimbs, nsets, (int)(k % 3), k % 5, 0)) return 1;
                k++;
            }
    // the packed counters of bits = 8: 1025 rows of 64 sets of 7 limbs (Fp) and of 16 sets of 31 limbs (Fp252) on one bin, and on the two bins
    // of one word -- one workgroup of the LDS form, 459 200 and 508 400 increments, flushed seven times and more; and the largest 32-bit histogram
    for (int shape : {1, 2}) {
        if (run_counts(ctx, MS_GOLDILOCKS_FP, 1, 1025, 8, 1, 7, 64, MS_EXT_ALWAYS, 3, shape)) return 1;
        if (run_counts(ctx, MS_STARK252_FP, 4, 1025, 8, 2, 31, 16, MS_EXT_ALWAYS, 0, shape)) return 1;
        if (run_counts(ctx, MS_GOLDILOCKS_FP, 1, 1025, 7, 3, 9, 64, MS_EXT_ALWAYS, 1, shape)) return 1;
    }
    for (int checked = 0; checked < 2; checked++) {                    // and once in checked mode, which scans the named columns first
        REQUIRE(ms_ctx_set_checked(ctx, checked) == MS_OK);
        if (run_columns(ctx, MS_STARK252_FP, 4, 300, 70, MS_EXT_IF_NONZERO)) return 1;
        if (run_counts(ctx, MS_STARK252_FP, 4, 300, 6, 3, 11, 3, MS_EXT_IF_ZERO, 2, 0)) return 1;
    }
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("bitwise sanitize ok\n");
    fflush(stdout);
    return 0;
}
