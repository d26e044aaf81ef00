// The device-resident public coin: PublicCoinImpl<F, H> (src/random.rs:61-141) behind the calls ProverChannel makes
// (src/channel.rs:46-100, src/fri.rs:217-247).  The state stays in HBM between calls, so a Merkle root is absorbed where the tree
// builder left it and a drawn challenge is read by the next kernel where the coin wrote it (ms_fri_fold_dev): the asynchronous entry
// points enqueue one single-wave launch and never wait.  Kernels and the rules they implement: coin_kernels.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_keccak.h"
#include "commit_host.h"
#include "coin_kernels.h"

using mscoin::State;
static_assert(sizeof(ms_coin_state) == sizeof(State), "ms_coin_state and its device image must agree");

// the hash of a coin created on this context, or MS_ERR_INVALID
static int coin_lookup(ms_ctx* ctx, const char* entry, const void* d_coin, int* hash) {
    if (!ctx || !d_coin) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->coins.find(const_cast<void*>(d_coin));
    if (it == ctx->coins.end()) return fail(MS_ERR_INVALID, "%s: d_coin was not returned by ms_coin_create on this context", entry);
    *hash = it->second;
    return MS_OK;
}

template <int OP>
static void launch_step(ms_ctx* ctx, int hash, void* d_coin, const void* d_digest, uint64_t arg, size_t count, void* d_out) {
    const dim3 one(1), wave(mscoin::WAVE);
    if (hash == MS_HASH_SHA256) hipLaunchKernelGGL((mscoin::coin_step<0, OP>), one, wave, 0, ctx->stream, (State*)d_coin, (const uint32_t*)d_digest, arg, count, (uint64_t*)d_out);
    else if (hash == MS_HASH_KECCAK256) hipLaunchKernelGGL((mscoin::coin_step<3, OP>), one, wave, 0, ctx->stream, (State*)d_coin, (const uint32_t*)d_digest, arg, count, (uint64_t*)d_out);
    else if (hash == MS_HASH_SHA3_256) hipLaunchKernelGGL((mscoin::coin_step<4, OP>), one, wave, 0, ctx->stream, (State*)d_coin, (const uint32_t*)d_digest, arg, count, (uint64_t*)d_out);
    else hipLaunchKernelGGL((mscoin::coin_step<1, OP>), one, wave, 0, ctx->stream, (State*)d_coin, (const uint32_t*)d_digest, arg, count, (uint64_t*)d_out);
}

template <int H>
static void launch_elements(ms_ctx* ctx, unsigned V, void* d_coin, const void* d_elems, size_t count) {
    const dim3 one(1), wave(mscoin::WAVE);
    State* c = (State*)d_coin;
    const uint64_t* e = (const uint64_t*)d_elems;
    if (V == 1) hipLaunchKernelGGL((mscoin::coin_reseed_elements<H, 1>), one, wave, 0, ctx->stream, c, e, count);
    else if (V == 3) hipLaunchKernelGGL((mscoin::coin_reseed_elements<H, 3>), one, wave, 0, ctx->stream, c, e, count);
    else hipLaunchKernelGGL((mscoin::coin_reseed_elements<H, 4>), one, wave, 0, ctx->stream, c, e, count);
}

static int write_state(ms_ctx* ctx, void* d_coin, const State& S) {          // the caller holds ctx->mu
    return stage_upload(ctx, d_coin, &S, sizeof S);
}

extern "C" int ms_coin_create(ms_ctx* ctx, int hash, const void* h_seed32, void** d_coin) {
    if (!ctx || !h_seed32 || !d_coin) return fail(MS_ERR_INVALID, "ms_coin_create: null argument");
    if (hash != MS_HASH_SHA256 && hash != MS_HASH_BLAKE2S && hash != MS_HASH_KECCAK256 && hash != MS_HASH_SHA3_256) return fail(MS_ERR_INVALID, "ms_coin_create: unknown hash id %d", hash);
    void* d = nullptr;
    MSCHK(ms_alloc(ctx, sizeof(State), &d));
    State S;
    memset(&S, 0, sizeof S);
    memcpy(S.seed, h_seed32, 32);
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int rc = write_state(ctx, d, S);
    if (rc != MS_OK) { (void)pool_free(ctx, d); return rc; }
    ctx->coins[d] = hash;
    *d_coin = d;
    return MS_OK;
}

extern "C" int ms_coin_destroy(ms_ctx* ctx, void* d_coin) {
    if (!ctx) return fail(MS_ERR_INVALID, "null context");
    if (!d_coin) return MS_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->coins.erase(d_coin)) return fail(MS_ERR_INVALID, "ms_coin_destroy: d_coin was not returned by ms_coin_create on this context");
    return pool_free(ctx, d_coin);
}

extern "C" int ms_coin_read(ms_ctx* ctx, const void* d_coin, void* h_state) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_read", d_coin, &hash));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_coin_read: null argument");
    return ms_download(ctx, h_state, d_coin, sizeof(State));
}

extern "C" int ms_coin_write(ms_ctx* ctx, void* d_coin, const void* h_state) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_write", d_coin, &hash));
    if (!h_state) return fail(MS_ERR_INVALID, "ms_coin_write: null argument");
    State S;
    memcpy(&S, h_state, sizeof S);
    if (S.nbytes > 32 || S.nbytes % 8) return fail(MS_ERR_INVALID, "ms_coin_write: nbytes = %u (the coin is read in whole words: 0, 8, 16, 24 or 32)", S.nbytes);
    S.pad = 0;
    memset((char*)S.unread + S.nbytes, 0, 32 - S.nbytes);                   // consumed bytes are kept cleared
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    return write_state(ctx, d_coin, S);
}

extern "C" int ms_coin_reseed_digest(ms_ctx* ctx, void* d_coin, const void* d_digest32) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_reseed_digest", d_coin, &hash));
    if (!d_digest32) return fail(MS_ERR_INVALID, "ms_coin_reseed_digest: null argument");
    if ((uintptr_t)d_digest32 & 3) return fail(MS_ERR_INVALID, "ms_coin_reseed_digest: d_digest32 must be 4-byte aligned");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "coin_reseed_digest", 0.0);
        launch_step<mscoin::OP_RESEED_DIGEST>(ctx, hash, d_coin, d_digest32, 0, 0, nullptr);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_coin_reseed_int(ms_ctx* ctx, void* d_coin, uint64_t value) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_reseed_int", d_coin, &hash));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "coin_reseed_int", 0.0);
        launch_step<mscoin::OP_RESEED_INT>(ctx, hash, d_coin, nullptr, value, 0, nullptr);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// the caller holds ctx->mu; d_elems is device-visible memory (a column, or a view of the staging ring)
static int reseed_elements_launch(ms_ctx* ctx, int hash, unsigned V, void* d_coin, const void* d_elems, size_t count) {
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "coin_reseed_elements", 8.0 * V * count);
        if (hash == MS_HASH_SHA256) launch_elements<0>(ctx, V, d_coin, d_elems, count);
        else if (hash == MS_HASH_KECCAK256) launch_elements<3>(ctx, V, d_coin, d_elems, count);
        else if (hash == MS_HASH_SHA3_256) launch_elements<4>(ctx, V, d_coin, d_elems, count);
        else launch_elements<1>(ctx, V, d_coin, d_elems, count);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_coin_reseed_elements(ms_ctx* ctx, void* d_coin, int field, const void* d_elems, size_t count) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_reseed_elements", d_coin, &hash));
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (count == 0) return MS_OK;                                           // reseeding with no element leaves counter and unread bytes alone
    if (!d_elems) return fail(MS_ERR_INVALID, "ms_coin_reseed_elements: null argument");
    MSCHK(canon_col(ctx, "ms_coin_reseed_elements", "d_elems", field, count, d_elems));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return reseed_elements_launch(ctx, hash, V, d_coin, d_elems, count);
}

extern "C" int ms_coin_reseed_elements_host(ms_ctx* ctx, void* d_coin, int field, const void* h_elems, size_t count) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_reseed_elements_host", d_coin, &hash));
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (count == 0) return MS_OK;
    if (!h_elems) return fail(MS_ERR_INVALID, "ms_coin_reseed_elements_host: null argument");
    MSCHK(canon_host(ctx, "ms_coin_reseed_elements_host", "h_elems", field, h_elems, count));
    std::lock_guard<std::mutex> lk(ctx->mu);
    LockedPoolGuard pooled(ctx);
    const void* d_view = nullptr;
    MSCHK(stage_view(ctx, h_elems, count * V * 8, &d_view, pooled));
    return reseed_elements_launch(ctx, hash, V, d_coin, d_view, count);
}

extern "C" int ms_coin_draw(ms_ctx* ctx, void* d_coin, int field, size_t count, void* d_out) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_draw", d_coin, &hash));
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (count == 0) return MS_OK;
    if (!d_out) return fail(MS_ERR_INVALID, "ms_coin_draw: null argument");
    if (ranges_overlap(d_out, count * V * 8, d_coin, sizeof(State))) return fail(MS_ERR_INVALID, "ms_coin_draw: d_out overlaps the coin's state");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "coin_draw", 8.0 * V * count);
        if (V == 4) launch_step<mscoin::OP_DRAW_FP252>(ctx, hash, d_coin, nullptr, 0, count, d_out);
        else launch_step<mscoin::OP_DRAW_FP>(ctx, hash, d_coin, nullptr, 0, count * V, d_out);      // Fq3: c0, c1, c2 in that order
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_coin_draw_queries(ms_ctx* ctx, void* d_coin, size_t max_n, size_t domain_size, uint64_t* h_positions, size_t* npos) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_draw_queries", d_coin, &hash));
    if (!npos || (max_n && !h_positions)) return fail(MS_ERR_INVALID, "ms_coin_draw_queries: null argument");
    if (domain_size == 0) return fail(MS_ERR_INVALID, "ms_coin_draw_queries: domain_size must be positive");
    *npos = 0;
    if (max_n == 0) return MS_OK;
    void* d_samples = nullptr;
    PoolGuard pooled(ctx);
    MSCHK(pooled.alloc(max_n * 8, &d_samples));
    std::vector<uint64_t> samples(max_n);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        HIPCHK(hipSetDevice(ctx->device));
        {
            ProfScope ps(ctx, "coin_draw_queries", 8.0 * max_n);
            launch_step<mscoin::OP_QUERIES>(ctx, hash, d_coin, nullptr, (uint64_t)domain_size, max_n, d_samples);
        }
        HIPCHK(hipGetLastError());
    }
    MSCHK(ms_download(ctx, samples.data(), d_samples, max_n * 8));
    std::sort(samples.begin(), samples.end());                             // the reference collects a BTreeSet: distinct, ascending
    samples.erase(std::unique(samples.begin(), samples.end()), samples.end());
    memcpy(h_positions, samples.data(), samples.size() * 8);
    *npos = samples.size();
    return MS_OK;
}

// the windowed search of commit_host.h; the kernel takes the seed from the coin's state
extern "C" int ms_coin_pow_grind(ms_ctx* ctx, void* d_coin, unsigned bits, uint64_t max_nonce, uint64_t* nonce) {
    int hash = 0;
    MSCHK(coin_lookup(ctx, "ms_coin_pow_grind", d_coin, &hash));
    if (!nonce) return fail(MS_ERR_INVALID, "ms_coin_pow_grind: null argument");
    return mscommit::grind_windows(ctx, bits, max_nonce, "coin_pow_grind", [&](unsigned long long base, unsigned long long count, unsigned long long* found) {
        const dim3 grid = mscommit::blocks_of(count, mscoin::NT), block(mscoin::NT);
        const State* coin = (const State*)d_coin;
        if (hash == MS_HASH_SHA256) hipLaunchKernelGGL(mscoin::coin_pow_grind<0>, grid, block, 0, ctx->stream, coin, base, count, bits, found);
        else if (hash == MS_HASH_KECCAK256) hipLaunchKernelGGL(mscoin::coin_pow_grind<3>, grid, block, 0, ctx->stream, coin, base, count, bits, found);
        else if (hash == MS_HASH_SHA3_256) hipLaunchKernelGGL(mscoin::coin_pow_grind<4>, grid, block, 0, ctx->stream, coin, base, count, bits, found);
        else hipLaunchKernelGGL(mscoin::coin_pow_grind<1>, grid, block, 0, ctx->stream, coin, base, count, bits, found);
    }, nonce);
}
