// The Poseidon public coin of the 252-bit field behind include/ministark_hip_hades_coin.h: one field element and a draw counter in HBM.
// As with ms_coin.cpp and ms_rpo_coin.cpp the state stays on the device between calls -- a root is absorbed where
// ms_poseidon252_merkle left it, a drawn challenge is read by ms_fri_fold_dev where the coin wrote it -- and the asynchronous entry
// points enqueue their launches and never wait.  ctx->hades_coins mirrors each record's n_draws: every change of it goes through this
// file, so a draw whose counters leave u64 is refused from the mirror, without reading the device.  Kernels and the rules they
// implement: hades_coin_kernels.h.  A translation unit of its own: ms_poseidon.cpp's kernels are compiled as they were.
#include "ms_internal.h"
#include "../../include/ministark_hip_hades_coin.h"
#include "commit_host.h"
#include "hades_coin_kernels.h"

using mshades::State;
static_assert(sizeof(ms_hades_coin_state) == sizeof(State), "ms_hades_coin_state and its device image must agree");

static int coin_lookup(ms_ctx* ctx, const char* entry, const void* d_coin) {
    if (!ctx || !d_coin) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->hades_coins.count(const_cast<void*>(d_coin))) return fail(MS_ERR_INVALID, "%s: d_coin was not returned by ms_hades_coin_create on this context", entry);
    return MS_OK;
}

static int coin_field(const char* entry, int field) {
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (field != MS_STARK252_FP) return fail(MS_ERR_UNSUPPORTED, "%s: this coin works over the 252-bit field (MS_STARK252_FP); Goldilocks draws from the RPO-256 coin", entry);
    return MS_OK;
}

// one single-lane launch for a whole reseed; the caller holds ctx->mu
static int enqueue_absorb(ms_ctx* ctx, const char* label, double bytes, void* d_coin, const void* d_in, uint64_t arg, size_t count, int op) {
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, label, bytes);
        hipLaunchKernelGGL(mshades::hades_coin_absorb, dim3(1), dim3(1), 0, ctx->stream, (State*)d_coin, (const uint64_t*)d_in, arg, count, op);
    }
    HIPCHK(hipGetLastError());
    ctx->hades_coins[d_coin] = 0;
    return MS_OK;
}

// `count` draws from the record's counter on; the caller holds ctx->mu.  One workgroup advances n_draws itself, behind its barrier;
// a longer grid is followed by the single-lane hades_coin_advance on the same stream.
static int enqueue_draw(ms_ctx* ctx, const char* entry, const char* label, double bytes, void* d_coin, size_t count, void* d_out, uint64_t qmask, int queries) {
    uint64_t& mirror = ctx->hades_coins[d_coin];
    if ((uint64_t)(count - 1) > ~0ull - mirror) return fail(MS_ERR_INVALID, "%s: n_draws = %llu and %zu more draws leave the u64 counter", entry, (unsigned long long)mirror, count);
    if (count > ((size_t)1 << 38)) return fail(MS_ERR_INVALID, "%s: at most 2^38 draws a call", entry);
    HIPCHK(hipSetDevice(ctx->device));
    const dim3 grid = mscommit::blocks_of(count, mshades::NT);
    const int bump = grid.x == 1;
    {
        ProfScope ps(ctx, label, bytes);
        hipLaunchKernelGGL(mshades::hades_coin_draw, grid, dim3(mshades::NT), 0, ctx->stream, (State*)d_coin, count, (uint64_t*)d_out, qmask, queries, bump);
        if (!bump) hipLaunchKernelGGL(mshades::hades_coin_advance, dim3(1), dim3(1), 0, ctx->stream, (State*)d_coin, (uint64_t)count);
    }
    HIPCHK(hipGetLastError());
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
    void* d = nullptr;
    MSCHK(ms_alloc(ctx, sizeof(State), &d));
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = hipSetDevice(ctx->device) == hipSuccess ? MS_OK : fail(MS_ERR_HIP, "ms_hades_coin_create: hipSetDevice");
    if (rc == MS_OK) rc = stage_upload(ctx, d, &S, sizeof S);
    if (rc != MS_OK) { (void)pool_free(ctx, d); return rc; }
    ctx->hades_coins[d] = 0;
    *d_coin = d;
    return MS_OK;
}

extern "C" int ms_hades_coin_destroy(ms_ctx* ctx, void* d_coin) {
    if (!ctx) return fail(MS_ERR_INVALID, "null context");
    if (!d_coin) return MS_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->hades_coins.erase(d_coin)) return fail(MS_ERR_INVALID, "ms_hades_coin_destroy: d_coin was not returned by ms_hades_coin_create on this context");
    return pool_free(ctx, d_coin);
}

extern "C" int ms_hades_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_read", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_hades_coin_read: null argument");
    return ms_download(ctx, h_state, d_coin, sizeof(State));
}

extern "C" int ms_hades_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_write", d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_hades_coin_write: null argument");
    State S;
    memcpy(&S, h_state, sizeof S);
    for (int q = 0; q < 4; q++)
        if (S.pad[q]) return fail(MS_ERR_INVALID, "ms_hades_coin_write: pad[%d] is not zero", q);
    f252::E d;
    memcpy(d.l, S.digest, 32);
    if (f252::geq_p(d)) return fail(MS_ERR_INVALID, "ms_hades_coin_write: digest is not below p");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    MSCHK(stage_upload(ctx, d_coin, &S, sizeof S));
    ctx->hades_coins[d_coin] = S.n_draws;
    return MS_OK;
}

extern "C" int ms_hades_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_reseed_digest", d_coin));
    if (!d_digest) return fail(MS_ERR_INVALID, "ms_hades_coin_reseed_digest: null argument");
    if ((uintptr_t)d_digest & 7) return fail(MS_ERR_INVALID, "ms_hades_coin_reseed_digest: d_digest must be 8-byte aligned");
    MSCHK(canon_col(ctx, "ms_hades_coin_reseed_digest", "d_digest", MS_STARK252_FP, 1, d_digest));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_absorb(ctx, "hades_coin_reseed_digest", 32.0, d_coin, d_digest, 0, 0, mshades::OP_RESEED_DIGEST);
}

extern "C" int ms_hades_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_reseed_int", d_coin));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_absorb(ctx, "hades_coin_reseed_int", 0.0, d_coin, nullptr, value, 0, mshades::OP_RESEED_INT);
}

extern "C" int ms_hades_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_reseed_elements", d_coin));
    MSCHK(coin_field("ms_hades_coin_reseed_elements", field));
    if (count == 0) return MS_OK;                                           // reseeding with no element leaves digest and n_draws alone
    if (!d_elems) return fail(MS_ERR_INVALID, "ms_hades_coin_reseed_elements: null argument");
    MSCHK(canon_col(ctx, "ms_hades_coin_reseed_elements", "d_elems", field, count, d_elems));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_absorb(ctx, "hades_coin_reseed_elements", 32.0 * count, d_coin, d_elems, 0, count, mshades::OP_RESEED_ELEMENTS);
}

extern "C" int ms_hades_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_reseed_elements_host", d_coin));
    MSCHK(coin_field("ms_hades_coin_reseed_elements_host", field));
    if (count == 0) return MS_OK;
    if (!h_elems) return fail(MS_ERR_INVALID, "ms_hades_coin_reseed_elements_host: null argument");
    MSCHK(canon_host(ctx, "ms_hades_coin_reseed_elements_host", "h_elems", field, h_elems, count));
    std::lock_guard<std::mutex> lk(ctx->mu);
    LockedPoolGuard pooled(ctx);
    const void* d_view = nullptr;
    MSCHK(stage_view(ctx, h_elems, count * 32, &d_view, pooled));
    return enqueue_absorb(ctx, "hades_coin_reseed_elements", 32.0 * count, d_coin, d_view, 0, count, mshades::OP_RESEED_ELEMENTS);
}

extern "C" int ms_hades_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_draw", d_coin));
    MSCHK(coin_field("ms_hades_coin_draw", field));
    if (count == 0) return MS_OK;
    if (!d_out) return fail(MS_ERR_INVALID, "ms_hades_coin_draw: null argument");
    if (ranges_overlap(d_out, count * 32, d_coin, sizeof(State))) return fail(MS_ERR_INVALID, "ms_hades_coin_draw: d_out overlaps the coin's state");
    std::lock_guard<std::mutex> lk(ctx->mu);
    return enqueue_draw(ctx, "ms_hades_coin_draw", "hades_coin_draw", 32.0 * count, d_coin, count, d_out, 0, 0);
}

extern "C" int ms_hades_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_draw_queries", d_coin));
    if (!npos || (max_n && !h_positions)) return fail(MS_ERR_INVALID, "ms_hades_coin_draw_queries: null argument");
    if (domain_size == 0 || (domain_size & (domain_size - 1)) || (uint64_t)domain_size > (1ull << 32))
        return fail(MS_ERR_INVALID, "ms_hades_coin_draw_queries: domain_size must be a power of two in 1..2^32");
    *npos = 0;
    if (max_n == 0) return MS_OK;
    void* d_samples = nullptr;
    PoolGuard pooled(ctx);
    MSCHK(pooled.alloc(max_n * 8, &d_samples));
    std::vector<uint64_t> samples(max_n);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(enqueue_draw(ctx, "ms_hades_coin_draw_queries", "hades_coin_draw_queries", 8.0 * max_n, d_coin, max_n, d_samples, (uint64_t)domain_size - 1, 1));
    }
    MSCHK(ms_download(ctx, samples.data(), d_samples, max_n * 8));
    std::sort(samples.begin(), samples.end());                             // distinct and ascending, as ms_coin_draw_queries returns them
    samples.erase(std::unique(samples.begin(), samples.end()), samples.end());
    memcpy(h_positions, samples.data(), samples.size() * 8);
    *npos = samples.size();
    return MS_OK;
}

// the windowed search of commit_host.h; the kernel takes the digest from the coin's state
extern "C" int ms_hades_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    MSCHK(coin_lookup(ctx, "ms_hades_coin_pow_grind", d_coin));
    if (!nonce) return fail(MS_ERR_INVALID, "ms_hades_coin_pow_grind: null argument");
    if (bits > 63) return fail(MS_ERR_INVALID, "ms_hades_coin_pow_grind: bits = %u (the condition is on one element's low bits: 0..63)", bits);
    return mscommit::grind_windows(ctx, bits, max_nonce, "hades_coin_pow_grind", [&](unsigned long long base, unsigned long long count, unsigned long long* found) {
        hipLaunchKernelGGL(mshades::hades_coin_pow_grind, mscommit::blocks_of(count, mshades::NT), dim3(mshades::NT), 0, ctx->stream, (const State*)d_coin, base, count, bits, found);
    }, nonce);
}
