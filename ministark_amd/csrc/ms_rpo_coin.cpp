// The RPO-256 public coin behind include/ministark_hip_rpo_coin.h: a 12-element sponge in HBM that absorbs and draws field elements.  As
// with ms_coin.cpp the state stays on the device between calls -- an RPO root is absorbed where ms_rpo256_merkle left it, a drawn challenge
// is read by ms_fri_fold_dev where the coin wrote it -- and the asynchronous entry points enqueue one single-wave launch and never wait.
// Kernels and the rules they implement: rpo_coin_kernels.h.  The registry, the argument checks and the tails shared with the other coins:
// coin_host.h; this file keeps the seed, the rules of ms_rpo_coin_write, the digest's scan and the launches.
#include "ms_internal.h"
#include "../../include/ministark_hip_rpo_coin.h"
#include "coin_host.h"
#include "rpo_coin_kernels.h"

using msrpocoin::State;
using msrpocoin::Wide;
using mscoinhost::RPO;
static_assert(sizeof(ms_rpo_coin_state) == sizeof(State), "ms_rpo_coin_state and its device image must agree");

// Fp or Fq3: the number of base-field words per element
static int coin_field(const char* entry, int field, unsigned* V) {
    MSCHK(field_words(field, V));
    if (*V == 4) return fail(MS_ERR_UNSUPPORTED, "%s: the RPO-256 coin works over Goldilocks (Fp or Fq3), not the 252-bit field", entry);
    return MS_OK;
}

template <int OP>
static int enqueue_step(ms_ctx* ctx, const char* label, double bytes, void* d_coin, const void* d_in, uint64_t arg, size_t count, void* d_out) {   // the caller holds ctx->mu
    return mscoinhost::enqueue(ctx, label, bytes, [&] {
        hipLaunchKernelGGL((msrpocoin::rpo_coin_step<Wide, OP>), dim3(1), dim3(msrpocoin::WAVE), 0, ctx->stream, (State*)d_coin, (const uint64_t*)d_in, arg, count, (uint64_t*)d_out);
    });
}

extern "C" int ms_rpo_coin_create(ms_ctx* ctx, const void* h_seed4, void** d_coin) {
    if (!ctx || !h_seed4 || !d_coin) return fail(MS_ERR_INVALID, "ms_rpo_coin_create: null argument");
    State S;
    memset(&S, 0, sizeof S);
    memcpy(&S.s[4], h_seed4, 32);
    for (int q = 4; q < 8; q++)
        if (S.s[q] >= gl::P) return fail(MS_ERR_INVALID, "ms_rpo_coin_create: seed word %d is not below p", q - 4);
    S.pos = 12;
    return mscoinhost::create(ctx, RPO, 0, &S, sizeof S, d_coin, [&](void* d) { return enqueue_step<msrpocoin::OP_CREATE>(ctx, "rpo_coin_create", 0.0, d, nullptr, 0, 0, nullptr); });
}

extern "C" int ms_rpo_coin_destroy(ms_ctx* ctx, void* d_coin) { return mscoinhost::destroy(ctx, RPO, "ms_rpo_coin_destroy", d_coin); }

extern "C" int ms_rpo_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state) { return mscoinhost::read(ctx, RPO, "ms_rpo_coin_read", d_coin, h_state, sizeof(State)); }

extern "C" int ms_rpo_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state) {
    MSCHK(mscoinhost::lookup(ctx, RPO, "ms_rpo_coin_write", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: null argument");
    State S;
    memcpy(&S, h_state, sizeof S);
    if (S.pos < 4 || S.pos > 12) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: pos = %u (the next unread rate element: 4..12)", S.pos);
    for (int q = 0; q < 7; q++)
        if (S.pad[q]) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: pad[%d] is not zero", q);
    for (int q = 0; q < 12; q++)
        if (S.s[q] >= gl::P) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: s[%d] is not below p", q);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return mscoinhost::upload(ctx, d_coin, &S, sizeof S);
}

extern "C" int ms_rpo_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest4) {
    MSCHK(mscoinhost::lookup(ctx, RPO, "ms_rpo_coin_reseed_digest", d_coin));
    if (!d_digest4) return fail(MS_ERR_INVALID, "ms_rpo_coin_reseed_digest: null argument");
    if ((uintptr_t)d_digest4 & 7) return fail(MS_ERR_INVALID, "ms_rpo_coin_reseed_digest: d_digest4 must be 8-byte aligned");
    MSCHK(canon_col(ctx, "ms_rpo_coin_reseed_digest", "d_digest4", MS_GOLDILOCKS_FP, 4, d_digest4));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<msrpocoin::OP_RESEED_DIGEST>(ctx, "rpo_coin_reseed_digest", 32.0, d_coin, d_digest4, 0, 0, nullptr);
}

extern "C" int ms_rpo_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value) {
    MSCHK(mscoinhost::lookup(ctx, RPO, "ms_rpo_coin_reseed_int", d_coin));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<msrpocoin::OP_RESEED_INT>(ctx, "rpo_coin_reseed_int", 0.0, d_coin, nullptr, value, 0, nullptr);
}

static int reseed_elements(ms_ctx* ctx, const char* entry, void* d_coin, int field, const void* elems, size_t count, bool host) {
    return mscoinhost::reseed_elements(ctx, RPO, entry, d_coin, field, elems, count, host, coin_field, [&](int, unsigned V, const void* d_elems, size_t n) {
        return enqueue_step<msrpocoin::OP_RESEED_ELEMENTS>(ctx, "rpo_coin_reseed_elements", 8.0 * V * n, d_coin, d_elems, 0, n * V, nullptr);
    });
}

extern "C" int ms_rpo_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count) {
    return reseed_elements(ctx, "ms_rpo_coin_reseed_elements", d_coin, field, d_elems, count, false);
}

extern "C" int ms_rpo_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count) {
    return reseed_elements(ctx, "ms_rpo_coin_reseed_elements_host", d_coin, field, h_elems, count, true);
}

extern "C" int ms_rpo_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out) {
    return mscoinhost::draw(ctx, RPO, "ms_rpo_coin_draw", d_coin, sizeof(State), field, count, d_out, coin_field, [&](int, unsigned V) {
        return enqueue_step<msrpocoin::OP_DRAW>(ctx, "rpo_coin_draw", 8.0 * V * count, d_coin, nullptr, 0, count * V, d_out);   // Fq3: c0, c1, c2 in that order
    });
}

extern "C" int ms_rpo_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos) {
    return mscoinhost::draw_queries(ctx, RPO, "ms_rpo_coin_draw_queries", d_coin, max_n, domain_size, true, h_positions, npos, [&](int, uint64_t mask, void* d_samples) {
        return enqueue_step<msrpocoin::OP_QUERIES>(ctx, "rpo_coin_draw_queries", 8.0 * max_n, d_coin, nullptr, mask, max_n, d_samples);
    });
}

// the kernel takes the sponge from the coin's state
extern "C" int ms_rpo_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    return mscoinhost::pow_grind(ctx, RPO, "ms_rpo_coin_pow_grind", "rpo_coin_pow_grind", d_coin, bits, "the condition is on one element", max_nonce, nonce, [&](int, unsigned long long base, unsigned long long count, unsigned long long* found) {
        hipLaunchKernelGGL(msrpocoin::rpo_coin_pow_grind, mscommit::blocks_of(count, msrpocoin::NT), dim3(msrpocoin::NT), 0, ctx->stream, (const State*)d_coin, base, count, bits, found);
    });
}
