// The RPO-256 public coin behind include/ministark_hip_rpo_coin.h: a 12-element sponge in HBM that absorbs and draws field elements.  As
// with ms_coin.cpp the state stays on the device between calls -- an RPO root is absorbed where ms_rpo256_merkle left it, a drawn challenge
// is read by ms_fri_fold_dev where the coin wrote it -- and the asynchronous entry points enqueue one single-wave launch and never wait.
// Kernels and the rules they implement: rpo_coin_kernels.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_rpo_coin.h"
#include "commit_host.h"
#include "rpo_coin_kernels.h"

using msrpocoin::State;
using msrpocoin::Wide;
static_assert(sizeof(ms_rpo_coin_state) == sizeof(State), "ms_rpo_coin_state and its device image must agree");

static int coin_lookup(ms_ctx* ctx, const char* entry, const void* d_coin) {
    if (!ctx || !d_coin) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->rpo_coins.count(const_cast<void*>(d_coin))) return fail(MS_ERR_INVALID, "%s: d_coin was not returned by ms_rpo_coin_create on this context", entry);
    return MS_OK;
}

// Fp or Fq3: the number of base-field words per element
static int coin_field(const char* entry, int field, unsigned* V) {
    MSCHK(field_words(field, V));
    if (*V == 4) return fail(MS_ERR_UNSUPPORTED, "%s: the RPO-256 coin works over Goldilocks (Fp or Fq3), not the 252-bit field", entry);
    return MS_OK;
}

template <int OP>
static void launch_step(ms_ctx* ctx, void* d_coin, const void* d_in, uint64_t arg, size_t count, void* d_out) {
    hipLaunchKernelGGL((msrpocoin::rpo_coin_step<Wide, OP>), dim3(1), dim3(msrpocoin::WAVE), 0, ctx->stream, (State*)d_coin, (const uint64_t*)d_in, arg, count, (uint64_t*)d_out);
}

template <int OP>
static int enqueue_step(ms_ctx* ctx, const char* label, double bytes, void* d_coin, const void* d_in, uint64_t arg, size_t count, void* d_out) {   // the caller holds ctx->mu
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, label, bytes);
        launch_step<OP>(ctx, d_coin, d_in, arg, count, d_out);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_rpo_coin_create(ms_ctx* ctx, const void* h_seed4, void** d_coin) {
    if (!ctx || !h_seed4 || !d_coin) return fail(MS_ERR_INVALID, "ms_rpo_coin_create: null argument");
    State S;
    memset(&S, 0, sizeof S);
    memcpy(&S.s[4], h_seed4, 32);
    for (int q = 4; q < 8; q++)
        if (S.s[q] >= gl::P) return fail(MS_ERR_INVALID, "ms_rpo_coin_create: seed word %d is not below p", q - 4);
    S.pos = 12;
    void* d = nullptr;
    MSCHK(ms_alloc(ctx, sizeof(State), &d));
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = stage_upload(ctx, d, &S, sizeof S);
    if (rc == MS_OK) rc = enqueue_step<msrpocoin::OP_CREATE>(ctx, "rpo_coin_create", 0.0, d, nullptr, 0, 0, nullptr);
    if (rc != MS_OK) { (void)pool_free(ctx, d); return rc; }
    ctx->rpo_coins[d] = 1;
    *d_coin = d;
    return MS_OK;
}

extern "C" int ms_rpo_coin_destroy(ms_ctx* ctx, void* d_coin) {
    if (!ctx) return fail(MS_ERR_INVALID, "null context");
    if (!d_coin) return MS_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->rpo_coins.erase(d_coin)) return fail(MS_ERR_INVALID, "ms_rpo_coin_destroy: d_coin was not returned by ms_rpo_coin_create on this context");
    return pool_free(ctx, d_coin);
}

extern "C" int ms_rpo_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_read", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_rpo_coin_read: null argument");
    return ms_download(ctx, h_state, d_coin, sizeof(State));
}

extern "C" int ms_rpo_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_write", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: null argument");
    State S;
    memcpy(&S, h_state, sizeof S);
    if (S.pos < 4 || S.pos > 12) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: pos = %u (the next unread rate element: 4..12)", S.pos);
    for (int q = 0; q < 7; q++)
        if (S.pad[q]) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: pad[%d] is not zero", q);
    for (int q = 0; q < 12; q++)
        if (S.s[q] >= gl::P) return fail(MS_ERR_INVALID, "ms_rpo_coin_write: s[%d] is not below p", q);
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    return stage_upload(ctx, d_coin, &S, sizeof S);
}

extern "C" int ms_rpo_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest4) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_reseed_digest", d_coin));
    if (!d_digest4) return fail(MS_ERR_INVALID, "ms_rpo_coin_reseed_digest: null argument");
    if ((uintptr_t)d_digest4 & 7) return fail(MS_ERR_INVALID, "ms_rpo_coin_reseed_digest: d_digest4 must be 8-byte aligned");
    MSCHK(canon_col(ctx, "ms_rpo_coin_reseed_digest", "d_digest4", MS_GOLDILOCKS_FP, 4, d_digest4));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<msrpocoin::OP_RESEED_DIGEST>(ctx, "rpo_coin_reseed_digest", 32.0, d_coin, d_digest4, 0, 0, nullptr);
}

extern "C" int ms_rpo_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_reseed_int", d_coin));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<msrpocoin::OP_RESEED_INT>(ctx, "rpo_coin_reseed_int", 0.0, d_coin, nullptr, value, 0, nullptr);
}

extern "C" int ms_rpo_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_reseed_elements", d_coin));
    unsigned V = 0;
    MSCHK(coin_field("ms_rpo_coin_reseed_elements", field, &V));
    if (count == 0) return MS_OK;                                           // reseeding with no element leaves state and pos alone
    if (!d_elems) return fail(MS_ERR_INVALID, "ms_rpo_coin_reseed_elements: null argument");
    MSCHK(canon_col(ctx, "ms_rpo_coin_reseed_elements", "d_elems", field, count, d_elems));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<msrpocoin::OP_RESEED_ELEMENTS>(ctx, "rpo_coin_reseed_elements", 8.0 * V * count, d_coin, d_elems, 0, count * V, nullptr);
}

extern "C" int ms_rpo_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_reseed_elements_host", d_coin));
    unsigned V = 0;
    MSCHK(coin_field("ms_rpo_coin_reseed_elements_host", field, &V));
    if (count == 0) return MS_OK;
    if (!h_elems) return fail(MS_ERR_INVALID, "ms_rpo_coin_reseed_elements_host: null argument");
    MSCHK(canon_host(ctx, "ms_rpo_coin_reseed_elements_host", "h_elems", field, h_elems, count));
    std::lock_guard<std::mutex> lk(ctx->mu);
    LockedPoolGuard pooled(ctx);
    const void* d_view = nullptr;
    MSCHK(stage_view(ctx, h_elems, count * V * 8, &d_view, pooled));
    return enqueue_step<msrpocoin::OP_RESEED_ELEMENTS>(ctx, "rpo_coin_reseed_elements", 8.0 * V * count, d_coin, d_view, 0, count * V, nullptr);
}

extern "C" int ms_rpo_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_draw", d_coin));
    unsigned V = 0;
    MSCHK(coin_field("ms_rpo_coin_draw", field, &V));
    if (count == 0) return MS_OK;
    if (!d_out) return fail(MS_ERR_INVALID, "ms_rpo_coin_draw: null argument");
    if (ranges_overlap(d_out, count * V * 8, d_coin, sizeof(State))) return fail(MS_ERR_INVALID, "ms_rpo_coin_draw: d_out overlaps the coin's state");
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_step<msrpocoin::OP_DRAW>(ctx, "rpo_coin_draw", 8.0 * V * count, d_coin, nullptr, 0, count * V, d_out);   // Fq3: c0, c1, c2 in that order
}

extern "C" int ms_rpo_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_draw_queries", d_coin));
    if (!npos || (max_n && !h_positions)) return fail(MS_ERR_INVALID, "ms_rpo_coin_draw_queries: null argument");
    if (domain_size == 0 || (domain_size & (domain_size - 1)) || (uint64_t)domain_size > (1ull << 32))
        return fail(MS_ERR_INVALID, "ms_rpo_coin_draw_queries: domain_size must be a power of two in 1..2^32");
    *npos = 0;
    if (max_n == 0) return MS_OK;
    void* d_samples = nullptr;
    PoolGuard pooled(ctx);
    MSCHK(pooled.alloc(max_n * 8, &d_samples));
    std::vector<uint64_t> samples(max_n);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(enqueue_step<msrpocoin::OP_QUERIES>(ctx, "rpo_coin_draw_queries", 8.0 * max_n, d_coin, nullptr, (uint64_t)domain_size - 1, max_n, d_samples));
    }
    MSCHK(ms_download(ctx, samples.data(), d_samples, max_n * 8));
    std::sort(samples.begin(), samples.end());                             // distinct and ascending, as ms_coin_draw_queries returns them
    samples.erase(std::unique(samples.begin(), samples.end()), samples.end());
    memcpy(h_positions, samples.data(), samples.size() * 8);
    *npos = samples.size();
    return MS_OK;
}

// the windowed search of commit_host.h; the kernel takes the sponge from the coin's state
extern "C" int ms_rpo_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    MSCHK(coin_lookup(ctx, "ms_rpo_coin_pow_grind", d_coin));
    if (!nonce) return fail(MS_ERR_INVALID, "ms_rpo_coin_pow_grind: null argument");
    if (bits > 63) return fail(MS_ERR_INVALID, "ms_rpo_coin_pow_grind: bits = %u (the condition is on one element: 0..63)", bits);
    return mscommit::grind_windows(ctx, bits, max_nonce, "rpo_coin_pow_grind", [&](unsigned long long base, unsigned long long count, unsigned long long* found) {
        hipLaunchKernelGGL(msrpocoin::rpo_coin_pow_grind, mscommit::blocks_of(count, msrpocoin::NT), dim3(msrpocoin::NT), 0, ctx->stream, (const State*)d_coin, base, count, bits, found);
    }, nonce);
}
