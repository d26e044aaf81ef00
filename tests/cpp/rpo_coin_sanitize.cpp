// Host code of the RPO-256 public coin (ministark_amd/csrc/ms_rpo_coin.cpp) under AddressSanitizer and UBSan, as a stand-alone CPU
// program: its own main, linked with the simulator build of the library's sources.  It walks every ms_rpo_coin_* entry point through
// its accepted and refused arguments -- handles, the staging ring of the host reseed, the sample buffer of the query draw, the
// search's windows -- and prints "rpo coin sanitize ok".  Not part of the suite (the build compiles every translation unit again);
// from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Iministark_amd/csrc -DMS_NO_JIT \
//       -DMS_EMU_DIR='"tests/emu"' -DMS_CSRC_DIR='"ministark_amd/csrc"' -Wno-unknown-pragmas ministark_amd/csrc/ms_*.cpp \
//       tests/emu/emu_runtime.cpp tests/cpp/rpo_coin_sanitize.cpp -o rpo_coin_sanitize -ldl && ./rpo_coin_sanitize
// The simulator keeps its fiber stacks in a pool for the life of the process (tests/emu/emu_runtime.cpp), which LeakSanitizer reports at
// exit: run with LSAN_OPTIONS=suppressions=FILE, FILE holding the line `leak:emu::run_block_threads`.  Nothing else is reported.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/ministark_hip_rpo_coin.h"

#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d): %s\n", #c, __LINE__, ms_last_error()); return 1; } } while (0)

int main() {
    ms_ctx* ctx = nullptr;
    REQUIRE(ms_ctx_create(0, &ctx) == MS_OK);
    const uint64_t P = 0xFFFFFFFF00000001ull;
    uint64_t seed[4] = {1, 2, 3, P - 1}, bad_seed[4] = {1, 2, P, 4};
    void *coin = nullptr, *other = nullptr, *byte_coin = nullptr;
    REQUIRE(ms_rpo_coin_create(ctx, bad_seed, &coin) == MS_ERR_INVALID && coin == nullptr);
    REQUIRE(ms_rpo_coin_create(ctx, nullptr, &coin) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_create(ctx, seed, &coin) == MS_OK && ms_rpo_coin_create(ctx, seed, &other) == MS_OK);
    uint8_t seed32[32] = {7};
    REQUIRE(ms_coin_create(ctx, MS_HASH_SHA256, seed32, &byte_coin) == MS_OK);
    REQUIRE(ms_rpo_coin_reseed_int(ctx, byte_coin, 1) == MS_ERR_INVALID && ms_coin_reseed_int(ctx, coin, 1) == MS_ERR_INVALID);

    ms_rpo_coin_state st, st2;
    REQUIRE(ms_rpo_coin_read(ctx, coin, &st) == MS_OK && st.pos == 4);
    REQUIRE(ms_rpo_coin_read(ctx, other, &st2) == MS_OK && !memcmp(&st, &st2, sizeof st));
    // host reseeds through the staging ring at the block edges, and a large one
    for (size_t count : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)65, (size_t)4096}) {
        std::vector<uint64_t> fp(count), fq3(3 * count);
        for (size_t i = 0; i < fp.size(); i++) fp[i] = (i * 0x9E3779B97F4A7C15ull) % P;
        for (size_t i = 0; i < fq3.size(); i++) fq3[i] = (i * 0xC2B2AE3D27D4EB4Full) % P;
        REQUIRE(ms_rpo_coin_reseed_elements_host(ctx, coin, MS_GOLDILOCKS_FP, fp.data(), count) == MS_OK);
        REQUIRE(ms_rpo_coin_reseed_elements_host(ctx, coin, MS_GOLDILOCKS_FQ3, fq3.data(), count) == MS_OK);
        // the device form on the same words gives the same state
        void* d = nullptr;
        REQUIRE(ms_alloc(ctx, 8 * (count ? count : 1), &d) == MS_OK);
        REQUIRE(ms_upload(ctx, d, fp.data(), 8 * count) == MS_OK);
        REQUIRE(ms_rpo_coin_reseed_elements(ctx, other, MS_GOLDILOCKS_FP, d, count) == MS_OK);
        REQUIRE(ms_free(ctx, d) == MS_OK);
        REQUIRE(ms_alloc(ctx, 24 * (count ? count : 1), &d) == MS_OK);
        REQUIRE(ms_upload(ctx, d, fq3.data(), 24 * count) == MS_OK);
        REQUIRE(ms_rpo_coin_reseed_elements(ctx, other, MS_GOLDILOCKS_FQ3, d, count) == MS_OK);
        REQUIRE(ms_free(ctx, d) == MS_OK);
        REQUIRE(ms_rpo_coin_read(ctx, coin, &st) == MS_OK && ms_rpo_coin_read(ctx, other, &st2) == MS_OK && !memcmp(&st, &st2, sizeof st));
    }
    REQUIRE(ms_rpo_coin_reseed_elements_host(ctx, coin, MS_STARK252_FP, seed, 1) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_rpo_coin_reseed_elements_host(ctx, coin, 9, seed, 1) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_reseed_elements_host(ctx, coin, MS_GOLDILOCKS_FP, nullptr, 1) == MS_ERR_INVALID);
    // draws of every length up to three blocks, into an exactly sized buffer
    for (size_t count = 0; count <= 25; count++) {
        void* d = nullptr;
        REQUIRE(ms_alloc(ctx, 24 * (count ? count : 1), &d) == MS_OK);
        REQUIRE(ms_rpo_coin_draw(ctx, coin, MS_GOLDILOCKS_FP, count, d) == MS_OK);
        REQUIRE(ms_rpo_coin_draw(ctx, coin, MS_GOLDILOCKS_FQ3, count, d) == MS_OK);
        std::vector<uint64_t> h(3 * count);
        REQUIRE(ms_download(ctx, h.data(), d, 24 * count) == MS_OK);
        for (uint64_t w : h) REQUIRE(w < P);
        REQUIRE(ms_free(ctx, d) == MS_OK);
    }
    REQUIRE(ms_rpo_coin_draw(ctx, coin, MS_GOLDILOCKS_FP, 1, coin) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_draw(ctx, coin, MS_STARK252_FP, 1, other) == MS_ERR_UNSUPPORTED);
    REQUIRE(ms_rpo_coin_reseed_digest(ctx, coin, other) == MS_OK);                       // any four canonical device words
    REQUIRE(ms_rpo_coin_reseed_digest(ctx, coin, (const char*)other + 4) == MS_ERR_INVALID);
    // query positions: exactly max_n slots
    for (size_t max_n : {(size_t)0, (size_t)1, (size_t)8, (size_t)100}) {
        std::vector<uint64_t> pos(max_n);
        size_t n = 99;
        REQUIRE(ms_rpo_coin_draw_queries(ctx, coin, max_n, 2, max_n ? pos.data() : nullptr, &n) == MS_OK && n <= 2 && n <= max_n);
        REQUIRE(ms_rpo_coin_draw_queries(ctx, coin, max_n, (size_t)1 << 32, max_n ? pos.data() : nullptr, &n) == MS_OK && n <= max_n);
        for (size_t i = 1; i < n; i++) REQUIRE(pos[i - 1] < pos[i]);
    }
    size_t n = 0; uint64_t one[1];
    REQUIRE(ms_rpo_coin_draw_queries(ctx, coin, 1, 3, one, &n) == MS_ERR_INVALID && ms_rpo_coin_draw_queries(ctx, coin, 1, 0, one, &n) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_draw_queries(ctx, coin, 1, (size_t)1 << 33, one, &n) == MS_ERR_INVALID);
    // the search: first window, a window cut short by max_nonce, no nonce, bits out of range; the state is left alone
    REQUIRE(ms_rpo_coin_read(ctx, coin, &st) == MS_OK);
    uint64_t nonce = 0, again = 0;
    REQUIRE(ms_rpo_coin_pow_grind(ctx, coin, 0, 1, &nonce) == MS_OK && nonce == 1);
    REQUIRE(ms_rpo_coin_pow_grind(ctx, coin, 10, 1 << 16, &nonce) == MS_OK && nonce >= 1);
    REQUIRE(ms_rpo_coin_pow_grind(ctx, coin, 10, nonce, &again) == MS_OK && again == nonce);
    if (nonce > 1) REQUIRE(ms_rpo_coin_pow_grind(ctx, coin, 10, nonce - 1, &again) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_pow_grind(ctx, coin, 64, 16, &again) == MS_ERR_INVALID && ms_rpo_coin_pow_grind(ctx, coin, 8, 16, nullptr) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_read(ctx, coin, &st2) == MS_OK && !memcmp(&st, &st2, sizeof st));
    REQUIRE(ms_rpo_coin_reseed_int(ctx, coin, nonce) == MS_OK && ms_rpo_coin_read(ctx, coin, &st) == MS_OK && st.pos == 4);
    // write: the refused records leave the state as it was
    st2 = st; st2.pos = 3;   REQUIRE(ms_rpo_coin_write(ctx, coin, &st2) == MS_ERR_INVALID);
    st2 = st; st2.pos = 13;  REQUIRE(ms_rpo_coin_write(ctx, coin, &st2) == MS_ERR_INVALID);
    st2 = st; st2.s[11] = P; REQUIRE(ms_rpo_coin_write(ctx, coin, &st2) == MS_ERR_INVALID);
    st2 = st; st2.pad[6] = 1; REQUIRE(ms_rpo_coin_write(ctx, coin, &st2) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_read(ctx, coin, &st2) == MS_OK && !memcmp(&st, &st2, sizeof st));
    st2.pos = 12; REQUIRE(ms_rpo_coin_write(ctx, coin, &st2) == MS_OK);
    REQUIRE(ms_rpo_coin_destroy(ctx, byte_coin) == MS_ERR_INVALID && ms_coin_destroy(ctx, coin) == MS_ERR_INVALID);
    REQUIRE(ms_rpo_coin_destroy(ctx, coin) == MS_OK && ms_rpo_coin_destroy(ctx, coin) == MS_ERR_INVALID && ms_rpo_coin_destroy(ctx, nullptr) == MS_OK);
    REQUIRE(ms_rpo_coin_read(ctx, coin, &st) == MS_ERR_INVALID);                         // a destroyed handle is no handle
    REQUIRE(ms_rpo_coin_destroy(ctx, other) == MS_OK && ms_coin_destroy(ctx, byte_coin) == MS_OK);
    REQUIRE(ms_ctx_destroy(ctx) == MS_OK);
    printf("rpo coin sanitize ok\n");
    return 0;
}
