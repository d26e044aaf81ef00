// The Poseidon public coin of the 252-bit field behind include/ministark_hip_hades_coin.h: one field element and a draw counter in HBM.
// As with ms_coin.cpp and ms_rpo_coin.cpp the state stays on the device between calls -- a root is absorbed where
// ms_poseidon252_merkle left it, a drawn challenge is read by ms_fri_fold_dev where the coin wrote it -- and the asynchronous entry
// points enqueue their launches and never wait.  The coin's record in ctx->coins mirrors n_draws: every change of it goes through this
// file, so a draw whose counters leave u64 is refused from the mirror, without reading the device.  Kernels and the rules they
// implement: hades_coin_kernels.h.  The registry, the argument checks and the tails shared with the other coins: coin_host.h.  A
// translation unit of its own: ms_poseidon.cpp's kernels are compiled as they were.
#include "ms_internal.h"
#include "../../include/ministark_hip_hades_coin.h"
#include "coin_host.h"
#include "hades_coin_kernels.h"

using mshades::State;
using mscoinhost::HADES;
static_assert(sizeof(ms_hades_coin_state) == sizeof(State), "ms_hades_coin_state and its device image must agree");

static int coin_field(const char* entry, int field, unsigned* V) {
    MSCHK(field_words(field, V));
    if (field != MS_STARK252_FP) return fail(MS_ERR_UNSUPPORTED, "%s: this coin works over the 252-bit field (MS_STARK252_FP); Goldilocks draws from the RPO-256 coin", entry);
    return MS_OK;
}

// one single-lane launch for a whole reseed; the caller holds ctx->mu
static int enqueue_absorb(ms_ctx* ctx, const char* label, double bytes, void* d_coin, const void* d_in, uint64_t arg, size_t count, int op) {
    MSCHK(mscoinhost::enqueue(ctx, label, bytes, [&] {
        hipLaunchKernelGGL(mshades::hades_coin_absorb, dim3(1), dim3(1), 0, ctx->stream, (State*)d_coin, (const uint64_t*)d_in, arg, count, op);
    }));
    ctx->coins[d_coin].n_draws = 0;
    return MS_OK;
}

// `count` draws from the record's counter on; the caller holds ctx->mu.  One workgroup advances n_draws itself, behind its barrier;
// a longer grid is followed by the single-lane hades_coin_advance on the same stream.
static int enqueue_draw(ms_ctx* ctx, const char* entry, const char* label, double bytes, void* d_coin, size_t count, void* d_out, uint64_t qmask, int queries) {
    uint64_t& mirror = ctx->coins[d_coin].n_draws;
    if ((uint64_t)(count - 1) > ~0ull - mirror) return fail(MS_ERR_INVALID, "%s: n_draws = %llu and %zu more draws leave the u64 counter", entry, (unsigned long long)mirror, count);
    if (count > ((size_t)1 << 38)) return fail(MS_ERR_INVALID, "%s: at most 2^38 draws a call", entry);
    const dim3 grid = mscommit::blocks_of(count, mshades::NT);
    const int bump = grid.x == 1;
    MSCHK(mscoinhost::enqueue(ctx, label, bytes, [&] {
        hipLaunchKernelGGL(mshades::hades_coin_draw, grid, dim3(mshades::NT), 0, ctx->stream, (State*)d_coin, count, (uint64_t*)d_out, qmask, queries, bump);
        if (!bump) hipLaunchKernelGGL(mshades::hades_coin_advance, dim3(1), dim3(1), 0, ctx->stream, (State*)d_coin, (uint64_t)count);
    }));
    mirror += count;
    return MS_OK;
}

extern "C" int ms_hades_coin_create(ms_ctx* ctx, const void* h_seed4, void** d_coin) {
    if (!ctx || !h_seed4 || !d_coin) return fail(MS_ERR_INVALID, "ms_hades_coin_create: null argument");
    f252::E seed;
    memcpy(seed.l, h_seed4, 32);
    if (f252::geq_p(seed)) return fail(MS_ERR_INVALID, "ms_hades_coin_create: the seed is not below p");
    State S;
    memset(&S, 0, sizeof S);
    const f252::E m = f252::to_mont(seed);
    memcpy(S.digest, m.l, 32);
    return mscoinhost::create(ctx, HADES, 0, &S, sizeof S, d_coin);
}

extern "C" int ms_hades_coin_destroy(ms_ctx* ctx, void* d_coin) { return mscoinhost::destroy(ctx, HADES, "ms_hades_coin_destroy", d_coin); }

extern "C" int ms_hades_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state) { return mscoinhost::read(ctx, HADES, "ms_hades_coin_read", d_coin, h_state, sizeof(State)); }

extern "C" int ms_hades_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state) {
    MSCHK(mscoinhost::lookup(ctx, HADES, "ms_hades_coin_write", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_hades_coin_write: null argument");
    State S;
    memcpy(&S, h_state, sizeof S);
    for (int q = 0; q < 4; q++)
        if (S.pad[q]) return fail(MS_ERR_INVALID, "ms_hades_coin_write: pad[%d] is not zero", q);
    f252::E d;
    memcpy(d.l, S.digest, 32);
    if (f252::geq_p(d)) return fail(MS_ERR_INVALID, "ms_hades_coin_write: digest is not below p");
    std::lock_guard<std::mutex> lk(ctx->mu);
    MSCHK(mscoinhost::upload(ctx, d_coin, &S, sizeof S));
    ctx->coins[d_coin].n_draws = S.n_draws;
    return MS_OK;
}

extern "C" int ms_hades_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest) {
    MSCHK(mscoinhost::lookup(ctx, HADES, "ms_hades_coin_reseed_digest", d_coin));
    if (!d_digest) return fail(MS_ERR_INVALID, "ms_hades_coin_reseed_digest: null argument");
    if ((uintptr_t)d_digest & 7) return fail(MS_ERR_INVALID, "ms_hades_coin_reseed_digest: d_digest must be 8-byte aligned");
    MSCHK(canon_col(ctx, "ms_hades_coin_reseed_digest", "d_digest", MS_STARK252_FP, 1, d_digest));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_absorb(ctx, "hades_coin_reseed_digest", 32.0, d_coin, d_digest, 0, 0, mshades::OP_RESEED_DIGEST);
}

extern "C" int ms_hades_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value) {
    MSCHK(mscoinhost::lookup(ctx, HADES, "ms_hades_coin_reseed_int", d_coin));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_absorb(ctx, "hades_coin_reseed_int", 0.0, d_coin, nullptr, value, 0, mshades::OP_RESEED_INT);
}

static int reseed_elements(ms_ctx* ctx, const char* entry, void* d_coin, int field, const void* elems, size_t count, bool host) {
    return mscoinhost::reseed_elements(ctx, HADES, entry, d_coin, field, elems, count, host, coin_field, [&](int, unsigned, const void* d_elems, size_t n) {
        return enqueue_absorb(ctx, "hades_coin_reseed_elements", 32.0 * n, d_coin, d_elems, 0, n, mshades::OP_RESEED_ELEMENTS);
    });
}

extern "C" int ms_hades_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count) {
    return reseed_elements(ctx, "ms_hades_coin_reseed_elements", d_coin, field, d_elems, count, false);
}

extern "C" int ms_hades_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count) {
    return reseed_elements(ctx, "ms_hades_coin_reseed_elements_host", d_coin, field, h_elems, count, true);
}

extern "C" int ms_hades_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out) {
    return mscoinhost::draw(ctx, HADES, "ms_hades_coin_draw", d_coin, sizeof(State), field, count, d_out, coin_field, [&](int, unsigned) {
        return enqueue_draw(ctx, "ms_hades_coin_draw", "hades_coin_draw", 32.0 * count, d_coin, count, d_out, 0, 0);
    });
}

extern "C" int ms_hades_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos) {
    return mscoinhost::draw_queries(ctx, HADES, "ms_hades_coin_draw_queries", d_coin, max_n, domain_size, true, h_positions, npos, [&](int, uint64_t mask, void* d_samples) {
        return enqueue_draw(ctx, "ms_hades_coin_draw_queries", "hades_coin_draw_queries", 8.0 * max_n, d_coin, max_n, d_samples, mask, 1);
    });
}

// the kernel takes the digest from the coin's state
extern "C" int ms_hades_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    return mscoinhost::pow_grind(ctx, HADES, "ms_hades_coin_pow_grind", "hades_coin_pow_grind", d_coin, bits, "the condition is on one element's low bits", max_nonce, nonce, [&](int, unsigned long long base, unsigned long long count, unsigned long long* found) {
        hipLaunchKernelGGL(mshades::hades_coin_pow_grind, mscommit::blocks_of(count, mshades::NT), dim3(mshades::NT), 0, ctx->stream, (const State*)d_coin, base, count, bits, found);
    });
}
