// The host side of a device-resident public coin, written once: the registry of the context's coins, create / destroy / read / upload, the
// enqueue of a launch, and the argument checks and tails of reseed_elements, draw, draw_queries and pow_grind.  ms_coin.cpp (the byte-hash
// coin), ms_rpo_coin.cpp and ms_hades_coin.cpp each keep what really differs -- the state struct, the seed and the rules of *_write, the
// digest's alignment and canonical scan, the launches -- and hand this layer small callables:
//   field(entry, field, &V)        the family's field rule: MS_OK and the words per element, or the refusal
//   launch(...)                    called with ctx->mu held; enqueues through enqueue() and returns its code
// Host-only: no kernel lives here.  `entry` is the entry point's name, for the error strings.
// Locking: ctx->mu is a plain mutex that canon_col, canon_host, ms_download, ms_alloc and PoolGuard take themselves, so lookup() releases it
// and it is taken again only around the upload or the enqueue.
#pragma once
#include "commit_host.h"

namespace mscoinhost {

enum Family { BYTE = 0, RPO = 1, HADES = 2 };
static const char* const CREATE[3] = {"ms_coin_create", "ms_rpo_coin_create", "ms_hades_coin_create"};

// a coin of `family` created on this context (and the byte coin's hash), or MS_ERR_INVALID: no family takes another's handle
static int lookup(ms_ctx* ctx, int family, const char* entry, const void* d_coin, int* hash = nullptr) {
    if (!ctx || !d_coin) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->coins.find(const_cast<void*>(d_coin));
    if (it == ctx->coins.end() || it->second.family != family) return fail(MS_ERR_INVALID, "%s: d_coin was not returned by %s on this context", entry, CREATE[family]);
    if (hash) *hash = it->second.hash;
    return MS_OK;
}

// the state's image to the device; the caller holds ctx->mu
static int upload(ms_ctx* ctx, void* d_coin, const void* h_state, size_t bytes) {
    HIPCHK(hipSetDevice(ctx->device));
    return stage_upload(ctx, d_coin, h_state, bytes);
}

// one ProfScope around launch() on the context's stream; the caller holds ctx->mu
template <class Launch>
static int enqueue(ms_ctx* ctx, const char* label, double bytes, Launch launch) {
    HIPCHK(hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, label, bytes);
        launch();
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// a new coin with the validated initial state; step(d) is what the family enqueues behind the upload (the RPO coin's first permutation)
template <class Step>
static int create(ms_ctx* ctx, int family, int hash, const void* h_state, size_t bytes, void** d_coin, Step step) {
    void* d = nullptr;
    MSCHK(ms_alloc(ctx, bytes, &d));
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = upload(ctx, d, h_state, bytes);
    if (rc == MS_OK) rc = step(d);
    if (rc != MS_OK) { (void)pool_free(ctx, d); return rc; }
    ctx->coins[d] = {family, hash, 0};
    *d_coin = d;
    return MS_OK;
}
static int create(ms_ctx* ctx, int family, int hash, const void* h_state, size_t bytes, void** d_coin) {
    return create(ctx, family, hash, h_state, bytes, d_coin, [](void*) { return MS_OK; });
}

// a refused destroy leaves the other family's coin registered and allocated
static int destroy(ms_ctx* ctx, int family, const char* entry, void* d_coin) {
    if (!ctx) return fail(MS_ERR_INVALID, "null context");
    if (!d_coin) return MS_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->coins.find(d_coin);
    if (it == ctx->coins.end() || it->second.family != family) return fail(MS_ERR_INVALID, "%s: d_coin was not returned by %s on this context", entry, CREATE[family]);
    ctx->coins.erase(it);
    return pool_free(ctx, d_coin);
}

static int read(ms_ctx* ctx, int family, const char* entry, const void* d_coin, void* h_state, size_t bytes) {
    MSCHK(lookup(ctx, family, entry, d_coin));
    if (!h_state) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    return ms_download(ctx, h_state, d_coin, bytes);
}

// reseed_elements (host = false: a device column) and reseed_elements_host (a view of the staging ring); launch(hash, V, d_elems, count)
template <class Field, class Launch>
static int reseed_elements(ms_ctx* ctx, int family, const char* entry, const void* d_coin, int fld, const void* elems, size_t count, bool host, Field field, Launch launch) {
    int hash = 0;
    MSCHK(lookup(ctx, family, entry, d_coin, &hash));
    unsigned V = 0;
    MSCHK(field(entry, fld, &V));
    if (count == 0) return MS_OK;                                           // reseeding with no element leaves the state alone
    if (!elems) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    MSCHK(host ? canon_host(ctx, entry, "h_elems", fld, elems, count) : canon_col(ctx, entry, "d_elems", fld, count, elems));
    std::lock_guard<std::mutex> lk(ctx->mu);
    LockedPoolGuard pooled(ctx);
    const void* d_elems = elems;
    if (host) MSCHK(stage_view(ctx, elems, count * V * 8, &d_elems, pooled));
    return launch(hash, V, d_elems, count);
}

// `count` elements of `fld` into d_out, which must not overlap the state_bytes of the coin; launch(hash, V)
template <class Field, class Launch>
static int draw(ms_ctx* ctx, int family, const char* entry, const void* d_coin, size_t state_bytes, int fld, size_t count, const void* d_out, Field field, Launch launch) {
    int hash = 0;
    MSCHK(lookup(ctx, family, entry, d_coin, &hash));
    unsigned V = 0;
    MSCHK(field(entry, fld, &V));
    if (count == 0) return MS_OK;
    if (!d_out) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    if (ranges_overlap(d_out, count * V * 8, d_coin, state_bytes)) return fail(MS_ERR_INVALID, "%s: d_out overlaps the coin's state", entry);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return launch(hash, V);
}

// max_n samples into a pooled buffer, then distinct and ascending on the host (the reference collects a BTreeSet).  The byte coin takes any
// positive domain_size and hands it to the kernel as it is; an algebraic coin (pow2) takes a power of two up to 2^32 and hands over the mask
// domain_size - 1.  launch(hash, that value, d_samples)
template <class Launch>
static int draw_queries(ms_ctx* ctx, int family, const char* entry, const void* d_coin, size_t max_n, size_t domain_size, bool pow2, uint64_t* h_positions, size_t* npos, Launch launch) {
    int hash = 0;
    MSCHK(lookup(ctx, family, entry, d_coin, &hash));
    if (!npos || (max_n && !h_positions)) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    if (!pow2 && domain_size == 0) return fail(MS_ERR_INVALID, "%s: domain_size must be positive", entry);
    if (pow2 && (domain_size == 0 || (domain_size & (domain_size - 1)) || (uint64_t)domain_size > (1ull << 32)))
        return fail(MS_ERR_INVALID, "%s: domain_size must be a power of two in 1..2^32", entry);
    *npos = 0;
    if (max_n == 0) return MS_OK;
    void* d_samples = nullptr;
    PoolGuard pooled(ctx);
    MSCHK(pooled.alloc(max_n * 8, &d_samples));
    std::vector<uint64_t> samples(max_n);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(launch(hash, (uint64_t)domain_size - (pow2 ? 1 : 0), d_samples));
    }
    MSCHK(ms_download(ctx, samples.data(), d_samples, max_n * 8));
    std::sort(samples.begin(), samples.end());
    samples.erase(std::unique(samples.begin(), samples.end()), samples.end());
    memcpy(h_positions, samples.data(), samples.size() * 8);
    *npos = samples.size();
    return MS_OK;
}

// the windowed search of commit_host.h, the kernel reading the coin's state; bits_rule, where the condition is on one element, is the
// refusal's wording for bits > 63.  launch(hash, base, count, found)
template <class Launch>
static int pow_grind(ms_ctx* ctx, int family, const char* entry, const char* label, const void* d_coin, unsigned bits, const char* bits_rule, uint64_t max_nonce, uint64_t* nonce, Launch launch) {
    int hash = 0;
    MSCHK(lookup(ctx, family, entry, d_coin, &hash));
    if (!nonce) return fail(MS_ERR_INVALID, "%s: null argument", entry);
    if (bits_rule && bits > 63) return fail(MS_ERR_INVALID, "%s: bits = %u (%s: 0..63)", entry, bits, bits_rule);
    return mscommit::grind_windows(ctx, bits, max_nonce, label, [&](unsigned long long base, unsigned long long count, unsigned long long* found) { launch(hash, base, count, found); }, nonce);
}

}  // namespace mscoinhost
