// The device-resident public coin: PublicCoinImpl<F, H> (src/random.rs:61-141) behind the calls ProverChannel makes
// (src/channel.rs:46-100, src/fri.rs:217-247).  The state stays in HBM between calls, so a Merkle root is absorbed where the tree
// builder left it and a drawn challenge is read by the next kernel where the coin wrote it (ms_fri_fold_dev): the asynchronous entry
// points enqueue one single-wave launch and never wait.  Kernels and the rules they implement: coin_kernels.h.  The registry, the argument
// checks and the tails shared with the two algebraic coins: coin_host.h; this file keeps the seed, the rules of ms_coin_write and the launches.
#include "ms_internal.h"
#include "../../include/ministark_hip_keccak.h"
#include "../../include/ministark_hip_blake3.h"
#include "coin_host.h"
#include "coin_kernels.h"

using mscoin::State;
using mscoinhost::BYTE;
static_assert(sizeof(ms_coin_state) == sizeof(State), "ms_coin_state and its device image must agree");

// f(std::integral_constant<int, H>) with H the kernels' hash index of MS_HASH_*: 0 SHA-256, 1 BLAKE2s, 3 Keccak-256, 4 SHA3-256, 6 BLAKE3
template <class F>
static void with_hash(int hash, F f) {
    if (hash == MS_HASH_SHA256) f(std::integral_constant<int, 0>());
    else if (hash == MS_HASH_KECCAK256) f(std::integral_constant<int, 3>());
    else if (hash == MS_HASH_SHA3_256) f(std::integral_constant<int, 4>());
    else if (hash == MS_HASH_BLAKE3) f(std::integral_constant<int, 6>());
    else f(std::integral_constant<int, 1>());
}

template <int OP>
static int enqueue_step(ms_ctx* ctx, const char* label, double bytes, int hash, void* d_coin, const void* d_digest, uint64_t arg, size_t count, void* d_out) {   // the caller holds ctx->mu
    return mscoinhost::enqueue(ctx, label, bytes, [&] {
        with_hash(hash, [&](auto h) {
            hipLaunchKernelGGL((mscoin::coin_step<decltype(h)::value, OP>), dim3(1), dim3(mscoin::WAVE), 0, ctx->stream, (State*)d_coin, (const uint32_t*)d_digest, arg, count, (uint64_t*)d_out);
        });
    });
}

static int any_field(const char*, int field, unsigned* V) { return field_words(field, V); }

extern "C" int ms_coin_create(ms_ctx* ctx, int hash, const void* h_seed32, void** d_coin) {
    if (!ctx || !h_seed32 || !d_coin) return fail(MS_ERR_INVALID, "ms_coin_create: null argument");
    if (hash != MS_HASH_SHA256 && hash != MS_HASH_BLAKE2S && hash != MS_HASH_KECCAK256 && hash != MS_HASH_SHA3_256 && hash != MS_HASH_BLAKE3) return fail(MS_ERR_INVALID, "ms_coin_create: unknown hash id %d", hash);
    State S;
    memset(&S, 0, sizeof S);
    memcpy(S.seed, h_seed32, 32);
    return mscoinhost::create(ctx, BYTE, hash, &S, sizeof S, d_coin);
}

extern "C" int ms_coin_destroy(ms_ctx* ctx, void* d_coin) { return mscoinhost::destroy(ctx, BYTE, "ms_coin_destroy", d_coin); }

extern "C" int ms_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state) { return mscoinhost::read(ctx, BYTE, "ms_coin_read", d_coin, h_state, sizeof(State)); }

extern "C" int ms_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state) {
    MSCHK(mscoinhost::lookup(ctx, BYTE, "ms_coin_write", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_coin_write: null argument");
    State S;
    memcpy(&S, h_state, sizeof S);
    if (S.nbytes > 32 || S.nbytes % 8) return fail(MS_ERR_INVALID, "ms_coin_write: nbytes = %u (the coin is read in whole words: 0, 8, 16, 24 or 32)", S.nbytes);
    S.pad = 0;
    memset((char*)S.unread + S.nbytes, 0, 32 - S.nbytes);                   // consumed bytes are kept cleared
    std::lock_guard<std::mutex> lk(ctx->mu);
    return mscoinhost::upload(ctx, d_coin, &S, sizeof S);
}

extern "C" int ms_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest32) {
    int hash = 0;
    MSCHK(mscoinhost::lookup(ctx, BYTE, "ms_coin_reseed_digest", d_coin, &hash));
    if (!d_digest32) return fail(MS_ERR_INVALID, "ms_coin_reseed_digest: null argument");
    if ((uintptr_t)d_digest32 & 3) return fail(MS_ERR_INVALID, "ms_coin_reseed_digest: d_digest32 must be 4-byte aligned");
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<mscoin::OP_RESEED_DIGEST>(ctx, "coin_reseed_digest", 0.0, hash, d_coin, d_digest32, 0, 0, nullptr);
}

extern "C" int ms_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value) {
    int hash = 0;
    MSCHK(mscoinhost::lookup(ctx, BYTE, "ms_coin_reseed_int", d_coin, &hash));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<mscoin::OP_RESEED_INT>(ctx, "coin_reseed_int", 0.0, hash, d_coin, nullptr, value, 0, nullptr);
}

// d_elems is device-visible memory: a column, or a view of the staging ring
static int reseed_elements(ms_ctx* ctx, const char* entry, void* d_coin, int field, const void* elems, size_t count, bool host) {
    return mscoinhost::reseed_elements(ctx, BYTE, entry, d_coin, field, elems, count, host, any_field, [&](int hash, unsigned V, const void* d_elems, size_t n) {
        return mscoinhost::enqueue(ctx, "coin_reseed_elements", 8.0 * V * n, [&] {
            with_hash(hash, [&](auto h) {
                constexpr int H = decltype(h)::value;
                const dim3 one(1), wave(mscoin::WAVE);
                State* c = (State*)d_coin;
                const uint64_t* e = (const uint64_t*)d_elems;
                if (V == 1) hipLaunchKernelGGL((mscoin::coin_reseed_elements<H, 1>), one, wave, 0, ctx->stream, c, e, n);
                else if (V == 3) hipLaunchKernelGGL((mscoin::coin_reseed_elements<H, 3>), one, wave, 0, ctx->stream, c, e, n);
                else hipLaunchKernelGGL((mscoin::coin_reseed_elements<H, 4>), one, wave, 0, ctx->stream, c, e, n);
            });
        });
    });
}

extern "C" int ms_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count) {
    return reseed_elements(ctx, "ms_coin_reseed_elements", d_coin, field, d_elems, count, false);
}

extern "C" int ms_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count) {
    return reseed_elements(ctx, "ms_coin_reseed_elements_host", d_coin, field, h_elems, count, true);
}

extern "C" int ms_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out) {
    return mscoinhost::draw(ctx, BYTE, "ms_coin_draw", d_coin, sizeof(State), field, count, d_out, any_field, [&](int hash, unsigned V) {
        if (V == 4) return enqueue_step<mscoin::OP_DRAW_FP252>(ctx, "coin_draw", 8.0 * V * count, hash, d_coin, nullptr, 0, count, d_out);
        return enqueue_step<mscoin::OP_DRAW_FP>(ctx, "coin_draw", 8.0 * V * count, hash, d_coin, nullptr, 0, count * V, d_out);      // Fq3: c0, c1, c2 in that order
    });
}

extern "C" int ms_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos) {
    return mscoinhost::draw_queries(ctx, BYTE, "ms_coin_draw_queries", d_coin, max_n, domain_size, false, h_positions, npos, [&](int hash, uint64_t domain, void* d_samples) {
        return enqueue_step<mscoin::OP_QUERIES>(ctx, "coin_draw_queries", 8.0 * max_n, hash, d_coin, nullptr, domain, max_n, d_samples);
    });
}

// the kernel takes the seed from the coin's state
extern "C" int ms_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    return mscoinhost::pow_grind(ctx, BYTE, "ms_coin_pow_grind", "coin_pow_grind", d_coin, bits, nullptr, max_nonce, nonce, [&](int hash, unsigned long long base, unsigned long long count, unsigned long long* found) {
        with_hash(hash, [&](auto h) {
            hipLaunchKernelGGL(mscoin::coin_pow_grind<decltype(h)::value>, mscommit::blocks_of(count, mscoin::NT), dim3(mscoin::NT), 0, ctx->stream, (const State*)d_coin, base, count, bits, found);
        });
    });
}
