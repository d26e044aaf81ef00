// NTT plans: the registry of the plans handed to the caller (ms_ntt_plan_create / ms_ntt_plan_destroy), the context's bounded plan cache,
// and every table a plan owns -- the twiddle tables of both fields, the two-pass LDE tables, the 2^18 inverse scale table.  Host code
// only: this unit launches nothing (ms_ntt.cpp and ms_ntt252.cpp run what is built here).
#include "ms_internal.h"
#include "ntt2_kernels.h"      // msntt2::TILE / TW: which passes of a plan are limb-form

#include <set>

static int plan_build(ms_ctx* ctx, unsigned V, unsigned log_n, bool inverse, uint64_t h, ms_ntt_plan** out);
static int plan_build252(ms_ctx* ctx, unsigned log_n, bool inverse, const f252::E& h, ms_ntt_plan** out);
static int plan_free(ms_ntt_plan* plan);

// ---------------------------------------------------------------------------------------
// plans handed to the caller
// ---------------------------------------------------------------------------------------
// Plan objects handed to the caller (ms_ntt_plan_create): a plan refers to its context (lock, stream, cached tables), so a
// context that is destroyed first releases them itself and takes them out of this registry; every entry point that receives
// a plan looks it up before touching it -- a plan destroyed after its context (a GpuFft collected after Planner.close()) is a
// no-op, a transform on it an error, never a read of freed memory -- for calls that do not RACE with the teardown: the lookup
// and the use that follows are two steps, so destroying a plan or its context on one thread while another thread is inside a
// call on that plan is outside the contract (include/ministark_hip.h, "Threads"), as it is for the reference's plans.
static std::mutex g_user_plans_mu;
static std::set<ms_ntt_plan*> g_user_plans;
bool user_plan_alive(ms_ntt_plan* p) { std::lock_guard<std::mutex> lk(g_user_plans_mu); return g_user_plans.count(p) != 0; }

// A handle: a copy of the cached plan `base` with a queue of its own (the caller holds ctx->mu)
static ms_ntt_plan* make_handle(ms_ntt_plan* base) {
    ms_ntt_plan* handle = new ms_ntt_plan(*base);
    handle->base = base; handle->refs = 0; handle->queue.clear(); handle->lde2.clear();
    base->refs++;
    return handle;
}
static int plan_create_impl(ms_ctx* ctx, int field, unsigned log_n, int inverse, const void* h_offset, const void* h_group_gen, ms_ntt_plan** out) {
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    MSCHK(canon_host(ctx, "ms_ntt_plan_create", "h_offset", V == 4 ? MS_STARK252_FP : MS_GOLDILOCKS_FP, h_offset, 1));      // twiddles are in Fp = F::FftField
    MSCHK(canon_host(ctx, "ms_ntt_plan_create", "h_group_gen", V == 4 ? MS_STARK252_FP : MS_GOLDILOCKS_FP, h_group_gen, 1));
    ms_ntt_plan* base = nullptr;
    if (V == 4) {
        // the 252-bit plans are cached per context like the Goldilocks ones (round 5: a handle used to build its own tables -- 2^18 powers
        // of a 252-bit root on the host, 6-16 ms per `GpuFft::from(domain)` in the reference's criterion harness, gpu/benches/fft.rs)
        if (log_n > 40) return fail(MS_ERR_INVALID, "log_n = %u too large", log_n);
        if (h_group_gen) {
            f252::E g; memcpy(g.l, h_group_gen, 32);
            if (!f252::eq(g, f252::root_of_unity(log_n))) return fail(MS_ERR_UNSUPPORTED, "group_gen is not arkworks' get_root_of_unity(2^%u)", log_n);
        }
        f252::E h;
        MSCHK(offset252(h_offset, &h));
        std::lock_guard<std::mutex> lk(ctx->mu);
        MSCHK(plan252_cached(ctx, log_n, inverse != 0, h, &base));
        *out = make_handle(base);
        return MS_OK;
    }
    if (log_n > 32) return fail(MS_ERR_INVALID, "log_n = %u exceeds the field's two-adicity (32)", log_n);
    if (h_group_gen) {
        uint64_t g_m;
        memcpy(&g_m, h_group_gen, 8);
        if (gl::from_mont(g_m) != gl::root_of_unity(log_n))
            return fail(MS_ERR_UNSUPPORTED, "group_gen is not arkworks' get_root_of_unity(2^%u)", log_n);
    }
    uint64_t h;
    MSCHK(offset_gl(h_offset, &h));
    std::lock_guard<std::mutex> lk(ctx->mu);
    MSCHK(ctx_plan(ctx, V, log_n, inverse != 0, h, &base));
    *out = make_handle(base);
    return MS_OK;
}
extern "C" int ms_ntt_plan_create(ms_ctx* ctx, int field, unsigned log_n, int inverse, const void* h_offset,
                                  const void* h_group_gen, ms_ntt_plan** out) {
    if (!ctx || !out) return fail(MS_ERR_INVALID, "ms_ntt_plan_create: null argument");
    MSCHK(plan_create_impl(ctx, field, log_n, inverse, h_offset, h_group_gen, out));
    std::lock_guard<std::mutex> lk(g_user_plans_mu);
    g_user_plans.insert(*out);
    return MS_OK;
}
void plans_release_ctx(ms_ctx* ctx) {
    std::vector<ms_ntt_plan*> mine;
    {
        std::lock_guard<std::mutex> lk(g_user_plans_mu);
        for (auto it = g_user_plans.begin(); it != g_user_plans.end();)
            if ((*it)->ctx == ctx) { mine.push_back(*it); it = g_user_plans.erase(it); } else ++it;
    }
    for (ms_ntt_plan* p : mine) (void)plan_free(p);
}
extern "C" int ms_ntt_plan_destroy(ms_ntt_plan* plan) {
    if (!plan) return MS_OK;
    {
        std::lock_guard<std::mutex> lk(g_user_plans_mu);
        if (!g_user_plans.erase(plan)) return MS_OK;               // released together with its context
    }
    return plan_free(plan);
}
int plan_free_cached(ms_ntt_plan* plan) { return plan_free(plan); }
// cached plans (owned by the context) and plans leaving the registry
static int plan_free(ms_ntt_plan* plan) {
    if (!plan) return MS_OK;
    if (plan->base) {                                              // a handle: the cached plan keeps the tables
        { std::lock_guard<std::mutex> lk(plan->ctx->mu); plan->base->refs--; }
        delete plan;
        return MS_OK;
    }
    (void)hipStreamSynchronize(plan->ctx->stream);
    ctx_side_sync(plan->ctx);
    if (plan->d_tables) (void)hipFree(plan->d_tables);
    if (plan->d_oscale) (void)hipFree(plan->d_oscale);
    for (auto& l : plan->lde2) if (l.d) (void)hipFree(l.d);
    delete plan;
    return MS_OK;
}

// ---------------------------------------------------------------------------------------
// the context's plan cache
// ---------------------------------------------------------------------------------------
// Plans owned by the context, reused by the fused entry points (ms_lde, ms_fri_fold, ...).  The cache is bounded:
// most recently used at the back, and beyond PLAN_CACHE_MAX entries the least recently used plan is destroyed
// (a prover that varies sizes / offsets -- FRI layers, periodic-column cosets -- would otherwise accumulate twiddle
// tables until ms_ctx_destroy).  One call uses at most a handful of plans, so a plan handed out in a call cannot
// be evicted by the same call.
static constexpr size_t PLAN_CACHE_MAX = 32;
static ms_ntt_plan* plan_cache_find(ms_ctx* ctx, unsigned V, unsigned log_n, bool inverse, uint64_t h, const uint64_t* off252 = nullptr) {
    auto& pc = ctx->plan_cache;
    for (size_t i = 0; i < pc.size(); i++) {
        const PlanKey& k = pc[i].first;
        if (k.V != V || k.log_n != log_n || k.inverse != inverse || k.h != h) continue;
        if (off252 && memcmp(pc[i].second->off252, off252, 32) != 0) continue;       // same hash, different offset
        auto hit = pc[i];
        pc.erase(pc.begin() + (long)i);
        pc.push_back(hit);
        return hit.second;
    }
    return nullptr;
}
static void plan_cache_insert(ms_ctx* ctx, const PlanKey& key, ms_ntt_plan* plan) {
    ctx->plan_cache.push_back({key, plan});
    while (ctx->plan_cache.size() > PLAN_CACHE_MAX) {
        size_t victim = 0;
        while (victim + 1 < ctx->plan_cache.size() && ctx->plan_cache[victim].second->refs > 0) victim++;   // least recently used plan without handles
        if (victim + 1 >= ctx->plan_cache.size()) break;       // everything older than the new plan is in use: let the cache grow
        ms_ntt_plan* old = ctx->plan_cache[victim].second;
        ctx->plan_cache.erase(ctx->plan_cache.begin() + (long)victim);
        (void)plan_free(old);                                  // synchronises the stream before freeing the tables
    }
}
int ctx_plan(ms_ctx* ctx, unsigned V, unsigned log_n, bool inverse, uint64_t h, ms_ntt_plan** out) {
    if ((*out = plan_cache_find(ctx, V, log_n, inverse, h)) != nullptr) return MS_OK;
    MSCHK(plan_build(ctx, V, log_n, inverse, h, out));
    plan_cache_insert(ctx, PlanKey{V, log_n, inverse, h}, *out);
    return MS_OK;
}
static uint64_t offset_key252(const f252::E& h) {
    uint64_t k = 1469598103934665603ull;
    for (int w = 0; w < 4; w++) { k ^= h.l[w]; k *= 1099511628211ull; }
    return k | ((uint64_t)1 << 63);
}
// Fp252: keyed by the offset itself (a non-zero canonical element: offset252)
int plan252_cached(ms_ctx* ctx, unsigned log_n, bool inverse, const f252::E& h, ms_ntt_plan** out) {
    const bool coset = !f252::eq(h, f252::one());
    const uint64_t key = coset ? offset_key252(h) : 1;
    if ((*out = plan_cache_find(ctx, 4, log_n, inverse, key, h.l)) != nullptr) return MS_OK;
    MSCHK(plan_build252(ctx, log_n, inverse, h, out));
    plan_cache_insert(ctx, PlanKey{4, log_n, inverse, key}, *out);
    return MS_OK;
}

// ---------------------------------------------------------------------------------------
// the tables of a plan
// ---------------------------------------------------------------------------------------
// All tables of a plan travel in one allocation, in the order they were added: add() appends a table and remembers which pointer of the
// plan is to point at it, upload() copies the lot and resolves those pointers.  A table that was never added stays null.
namespace {
struct PlanTables {
    std::vector<uint64_t> host;
    std::vector<std::pair<uint64_t**, size_t>> slots;
    void add(uint64_t*& slot, const std::vector<uint64_t>& t) {
        slots.push_back({&slot, host.size()});
        host.insert(host.end(), t.begin(), t.end());
    }
    // the tables of the limb-form passes (ntt2_kernels.h): plain residues, four copies {w, w 2^24, w 2^48, w 2^72} per twiddle
    void add4(uint64_t*& slot, const std::vector<uint64_t>& plain) {
        static const uint64_t sh[4] = {1, (uint64_t)1 << 24, (uint64_t)1 << 48, gl::pow(2, 72)};
        slots.push_back({&slot, host.size()});
        host.reserve(host.size() + 4 * plain.size());
        for (uint64_t v : plain) for (int i = 0; i < 4; i++) host.push_back(gl::mul(v, sh[i]));
    }
    // on failure the plan is deleted
    int upload(ms_ntt_plan* p, const char* what) {
        hipError_t e = hipMalloc(&p->d_tables, host.size() * 8);
        if (e != hipSuccess) { delete p; return fail(MS_ERR_NOMEM, "%s tables (%zu bytes): %s", what, host.size() * 8, hipGetErrorString(e)); }
        e = hipMemcpy(p->d_tables, host.data(), host.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p->d_tables); delete p; return fail(MS_ERR_HIP, "%s table upload: %s", what, hipGetErrorString(e)); }
        for (auto& s : slots) *s.first = p->d_tables + s.second;
        return MS_OK;
    }
};
}  // namespace

static void powers(std::vector<uint64_t>& out, size_t count, uint64_t base, uint64_t first = 1) {
    out.resize(count);
    uint64_t x = first;
    for (size_t i = 0; i < count; i++) { out[i] = x; x = gl::mul(x, base); }
}
static void powers252(std::vector<uint64_t>& out, size_t count, f252::E base, f252::E first) {
    out.resize(count * 4);
    f252::E x = first;
    for (size_t i = 0; i < count; i++) { memcpy(&out[4 * i], x.l, 32); x = f252::mul(x, base); }
}

// ---- Fp252 plans ------------------------------------------------------------------------
// h: the coset offset, a non-zero canonical element (offset252)
static int plan_build252(ms_ctx* ctx, unsigned log_n, bool inverse, const f252::E& h, ms_ntt_plan** out) {
    HIPCHK(hipSetDevice(ctx->device));
    const f252::E gen = f252::root_of_unity(log_n);
    const bool coset = !f252::eq(h, f252::one());
    ms_ntt_plan* p = new ms_ntt_plan();
    p->ctx = ctx; p->V = 4; p->log_n = log_n; p->inverse = inverse; p->coset = coset; p->is252 = true;
    memcpy(p->off252, h.l, 32);
    const size_t n = (size_t)1 << log_n;
    const f252::E w = inverse ? f252::inv(gen) : gen;
    // one-level tables up to 2^21 points: every twiddle / scale factor is a single 32-byte load.  (A two-level
    // lookup costs a second Montgomery product per butterfly, and the product -- ~440 VALU instructions -- is
    // what bounds this field.)  Larger domains split the exponent at 2^21.
    p->lo_bits = std::min(21u, log_n);
    PlanTables T;
    std::vector<uint64_t> t;
    powers252(t, (size_t)1 << p->lo_bits, w, f252::one()); T.add(p->d252_tw_lo, t);
    powers252(t, std::max<size_t>(n >> p->lo_bits, 1), f252::pow_u64(w, (uint64_t)1 << p->lo_bits), f252::one()); T.add(p->d252_tw_hi, t);
    if (inverse || coset) {
        f252::E g = inverse ? f252::inv(h) : h, c = f252::one();
        if (inverse) { f252::E nn = f252::to_mont(f252::E{{(uint64_t)n, 0, 0, 0}}); c = f252::inv(nn); }
        powers252(t, (size_t)1 << p->lo_bits, g, c); T.add(p->d252_sc_lo, t);
        powers252(t, std::max<size_t>(n >> p->lo_bits, 1), f252::pow_u64(g, (uint64_t)1 << p->lo_bits), f252::one()); T.add(p->d252_sc_hi, t);
        if (inverse) p->scale_out252 = 1; else p->scale_in252 = 1;
    }
    if (log_n >= NTT252_TILE_LOG && log_n <= 30) {
        p->np252 = log_n <= 20 ? 2 : 3;
        // MS_NTT252_PASSES=3 forces the three-pass split from 2^17 points on (tests: the emulator cannot hold 2^21 points)
        if (const char* e = getenv("MS_NTT252_PASSES")) if (atoi(e) == 3 && log_n >= 17) p->np252 = 3;
        for (int q = 0; q < p->np252; q++) p->lr252[q] = log_n / p->np252 + ((unsigned)q < log_n % p->np252 ? 1 : 0);
        for (int q = 0; q < p->np252; q++) {
            powers252(t, (size_t)1 << (p->lr252[q] - 1), f252::pow_u64(w, (uint64_t)n >> p->lr252[q]), f252::one());
            T.add(p->d252_twr[q], t);
        }
    }
    MSCHK(T.upload(p, "Fp252 plan"));
    *out = p;
    return MS_OK;
}

// ---- Goldilocks plans -------------------------------------------------------------------
// rev(U) of a middle pass q: the tile index U with its digit fields swapped back into the order of the exponent
static unsigned tile_exponent(const ms_ntt_plan* p, int q, unsigned U) {
    unsigned rU = 0;
    for (unsigned f = 0; f < p->nfields[q]; f++)
        rU |= ((U >> p->fields[q][f].in_shift) & p->fields[q][f].mask) << p->fields[q][f].out_shift;
    return rU;
}
static int plan_build(ms_ctx* ctx, unsigned V, unsigned log_n, bool inverse, uint64_t h, ms_ntt_plan** out) {
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t gen = gl::root_of_unity(log_n);           // plain, arkworks get_root_of_unity
    ms_ntt_plan* p = new ms_ntt_plan();
    p->ctx = ctx; p->V = V; p->log_n = log_n; p->inverse = inverse; p->coset = (h != 1); p->offset_canon = h;
    const size_t n = (size_t)1 << log_n;
    const uint64_t w = p->inverse ? gl::inv(gen) : gen;       // transform root
    const uint64_t hinv = gl::inv(h);
    const uint64_t ninv = gl::inv((uint64_t)(n % gl::P));
    const bool fwd_coset = !p->inverse && p->coset;

    PlanTables T;
    std::vector<uint64_t> t;
    if (log_n < 12) {
        p->small = true;
        powers(t, std::max<size_t>(n / 2, 1), w); T.add(p->d_tw, t);
        if (fwd_coset) { powers(t, n, h); T.add(p->d_scale_in, t); }
        if (p->inverse) { powers(t, n, hinv, ninv); T.add(p->d_scale_out, t); }
    }
    // Fp columns of 2^11 points ALSO get the tables of the (256, 8) plan: their dense transforms run as ntt_fused_tiny (ntt_kernels.h: two columns
    // per workgroup), everything else of a small plan (Fq3 columns, zero-extended inputs) stays with ntt_small.  Measured, 512 columns, forward /
    // inverse (profiles/r06_c2_sweep_small.json): 2^11 0.103 / 0.101 -> 0.135 / 0.127 of HBM and 29.4 -> 27.3 us for one column.  At 2^10 and 2^9
    // the same kernel (four and eight columns per workgroup) LOSES to ntt_small, 0.085 -> 0.072 and 0.055 -> 0.035: a batch of such columns is a
    // handful of workgroups whose time is their own latency, and ntt_small's ten cheap stages are the shorter chain there.  Not used below 2^11.
    p->tiny_fused = log_n == 11 && V == 1;
    if (log_n >= 12 || p->tiny_fused) {
        // radix decomposition: R1 = 256, the rest split as evenly as possible into radices 16..256
        const unsigned rest = log_n - 8;
        const int extra = (int)((rest + 7) / 8);
        p->npass = 1 + extra;
        p->lr[0] = 8;
        for (int i = 0; i < extra; i++) p->lr[1 + i] = rest / extra + ((unsigned)i < rest % extra ? 1 : 0);
        // three passes (2^17..2^24): (256, R, 256) with R = n / 2^16 -- both outer passes are the limb-form radix-256 kernels with
        // the uniform inter-pass factor (ntt2_kernels.h), so the last pass always has its limb-form variants (scale of an inverse
        // coset transform, fused bit-reversed store); the small radix sits in the middle: R <= 16 holds its whole network in
        // registers (ntt2_small_mid_pass), R = 32..128 is ntt2_mid_pass_r, R = 256 ntt2_mid_pass
        if (rest >= 9 && rest <= 16) { p->npass = 3; p->lr[1] = rest - 8; p->lr[2] = 8; }
        unsigned acc = 0;
        for (int q = 0; q < p->npass; q++) { p->log_s[q] = acc; acc += p->lr[q]; }
        // digit fields.  pass 1 maps j' = (j2..jm) [jm least significant] to layout (jm..j2) [j2 least]
        {
            unsigned nf = 0, in_shift = 0;
            for (int q = p->npass - 1; q >= 1; q--) {            // jm first (least significant of j')
                unsigned out_shift = 0;
                for (int r = 1; r < q; r++) out_shift += p->lr[r];
                p->fields[0][nf++] = {in_shift, out_shift, (1u << p->lr[q]) - 1};
                in_shift += p->lr[q];
            }
            p->nfields[0] = nf;
        }
        // pass q (0-based, 1 <= q < npass-1): U = (jm..j_{q+2}) [j_{q+2} least significant in U]
        //   -> j' = (j_{q+2}, ..., jm) [jm least significant]
        for (int q = 1; q < p->npass - 1; q++) {
            unsigned nf = 0, in_shift = 0;
            for (int r = q + 1; r < p->npass; r++) {             // r = digit index (0-based) above q
                unsigned out_shift = 0;
                for (int r2 = r + 1; r2 < p->npass; r2++) out_shift += p->lr[r2];
                p->fields[q][nf++] = {in_shift, out_shift, (1u << p->lr[r]) - 1};
                in_shift += p->lr[r];
            }
            p->nfields[q] = nf;
        }
        p->lo_bits = std::min(12u, log_n);
        powers(t, (size_t)1 << p->lo_bits, w); T.add(p->d_tw_lo, t);
        powers(t, n >> p->lo_bits, gl::pow(w, (uint64_t)1 << p->lo_bits)); T.add(p->d_tw_hi, t);
        for (int q = 0; q < p->npass; q++) {
            powers(t, (size_t)1 << p->lr[q], gl::pow(w, (uint64_t)n >> p->lr[q])); T.add(p->d_wr[q], t);
        }
        if (fwd_coset) {
            powers(t, (size_t)1 << p->lo_bits, h); T.add(p->d_aux_lo, t);
            powers(t, std::max<size_t>((n >> 8) >> p->lo_bits, 1), gl::pow(h, (uint64_t)1 << p->lo_bits)); T.add(p->d_aux_hi, t);
            powers(t, 256, gl::pow(h, (uint64_t)(n >> 8))); T.add(p->d_gtab, t);
        }
        if (p->inverse) {
            if (!p->coset) { p->scale_mode = 1; p->scale_const = ninv; }
            else {
                p->scale_mode = 2;
                powers(t, (size_t)1 << p->lo_bits, hinv, ninv); T.add(p->d_aux_lo, t);
                powers(t, n >> p->lo_bits, gl::pow(hinv, (uint64_t)1 << p->lo_bits)); T.add(p->d_aux_hi, t);
            }
        }
    }
    // device tables are in Montgomery form: gld::mmul(data, w * 2^64) = data * w
    for (auto& v : T.host) v = gl::to_mont(v);
    // ... except the tables of the limb-form passes (add4) and d_lq: plain residues, appended after the conversion
    p->uni = !p->small && p->npass == 3 && (p->lr[1] == 8 || p->lr[2] == 8) && p->lr[2] >= 6 && (n * V) % msntt2::TILE == 0;
    if (!p->small) {
        for (int q = 0; q < p->npass; q++) {
            const bool small_mid = p->uni && q == 1 && p->lr[q] < 8;       // ntt2_small_mid_pass / ntt2_mid_pass_r: [U][k2], k2 < R
            if (p->lr[q] != 8 && !small_mid) continue;
            if (!small_mid) { powers(t, 256, gl::pow(w, (uint64_t)n >> 8)); T.add4(p->d_wr4[q], t); }
            else if (p->lr[q] > 4) {                                       // ntt2_mid_pass_r: w_R^e, e < R = 16 T2 (it needs e = a' b < 16 T2)
                powers(t, (size_t)1 << p->lr[q], gl::pow(w, (uint64_t)n >> p->lr[q]));
                T.add4(p->d_wr4[q], t);
            }
            if (q >= 1 && q < p->npass - 1) {
                // w_U^k = w_n^((rev(U) k) << log_s): the factor ntt_mid_pass builds per tile in LDS (twl[])
                const size_t R = (size_t)1 << p->lr[q];
                const size_t nU = n >> (p->lr[q] + p->log_s[q]);
                const uint64_t ws = gl::pow(w, (uint64_t)1 << p->log_s[q]);
                t.resize(nU * R);
                for (size_t U = 0; U < nU; U++) {
                    const unsigned rU = tile_exponent(p, q, (unsigned)U);
                    const uint64_t wu = gl::pow(ws, rU);
                    // UNI plans: pass 2 also carries h^j3 of the inter-pass factor (h w_n^k1)^(R3 j2 + j3), j3 = rev(U)
                    uint64_t x = (p->uni && q == 1 && fwd_coset) ? gl::pow(h, rU) : 1;
                    // ntt2_mid_pass (radix 256) reads it in wave order: k = a' + 16 d sits at 16 a' + d, a wave's 16 factors of a round in a row
                    for (size_t k = 0; k < R; k++) { t[U * R + (small_mid ? k : (k & 15) * 16 + (k >> 4))] = x; x = gl::mul(x, wu); }
                }
                T.add4(p->d_twu4[q], t);
            }
        }
        t.assign(1, ninv); T.add4(p->d_sc4, t);
        if (p->scale_mode == 2 && p->lr[p->npass - 1] == 8) {      // inverse coset, last radix 256: h^-(k 2^log_s) per output row
            powers(t, 256, gl::pow(hinv, (uint64_t)1 << p->log_s[p->npass - 1])); T.add4(p->d_scu4, t);
        }
        if (p->uni) {
            // pass 1: tin4[j2][b][a'] = w_256^(a' b) w_n^(a' R3 j2) = w_n^(a' (b n/256 + R3 j2));
            //         tout4[j2][b'] = h^(R3 j2) w_n^(16 b' R3 j2)      (h = 1 unless this is a forward coset transform)
            const unsigned r3 = p->lr[2];
            const unsigned R2 = 1u << p->lr[1];
            const uint64_t hh = fwd_coset ? h : 1;
            t.resize((size_t)R2 * 256);
            for (unsigned j2 = 0; j2 < R2; j2++)
                for (unsigned b = 0; b < 16; b++) {
                    const uint64_t m = ((uint64_t)b * (n >> 8) + ((uint64_t)j2 << r3)) & (n - 1);
                    const uint64_t wm = gl::pow(w, m);
                    uint64_t x = 1;
                    for (unsigned a = 0; a < 16; a++) { t[((size_t)j2 * 16 + b) * 16 + a] = x; x = gl::mul(x, wm); }
                }
            T.add4(p->d_tin4, t);
            t.resize((size_t)R2 * 16);
            for (unsigned j2 = 0; j2 < R2; j2++) {
                const uint64_t wm = gl::pow(w, (((uint64_t)j2 << r3) * 16) & (n - 1));
                uint64_t x = gl::pow(hh, (uint64_t)j2 << r3);
                for (unsigned bp = 0; bp < 16; bp++) { t[(size_t)j2 * 16 + bp] = x; x = gl::mul(x, wm); }
            }
            T.add4(p->d_tout4, t);
            if (p->V == 1 && p->lr[1] == 8) {
                // pass 2 (ntt2_mid_pass<.., PERM>): lq[U][k1] = w_n^(k1 rev(U)), the per-lane factor on its loads as one plain word
                const unsigned nU = 1u << p->lr[2];              // blocks of 256 rows; a row is 2^log_s[1] = 256 words
                t.resize((size_t)nU * 256);
                for (unsigned U = 0; U < nU; U++) {
                    const uint64_t wu = gl::pow(w, tile_exponent(p, 1, U));
                    uint64_t x = 1;
                    for (unsigned k1 = 0; k1 < 256; k1++) { t[(size_t)U * 256 + k1] = x; x = gl::mul(x, wu); }
                }
                T.add(p->d_lq, t);
            }
        }
        if (fwd_coset) { powers(t, 256, gl::pow(h, (uint64_t)(n >> 8))); T.add4(p->d_g4, t); }
    }
    p->scale_const = gl::to_mont(p->scale_const);
    MSCHK(T.upload(p, "plan"));
    *out = p;
    return MS_OK;
}

// ---- the 2^18 inverse scale table ---------------------------------------------------------
// n^-1 h^-k, k < n = 2^18 (Montgomery), for the two-pass route of an inverse coset transform: built once per CACHED plan (`owner`:
// a handle is a copy that may predate the table).  The caller holds ctx->mu.
int plan_oscale(ms_ntt_plan* owner) {
    if (!owner->coset || owner->d_oscale) return MS_OK;
    const size_t n18 = (size_t)1 << 18;
    std::vector<uint64_t> sc(n18);
    const uint64_t hinv = gl::inv(owner->offset_canon);
    uint64_t x = gl::inv((uint64_t)n18);
    for (size_t k = 0; k < n18; k++) { sc[k] = gl::to_mont(x); x = gl::mul(x, hinv); }
    uint64_t* d = nullptr;
    if (hipMalloc(&d, n18 * 8) != hipSuccess) return fail(MS_ERR_NOMEM, "inverse scale table");
    if (hipMemcpy(d, sc.data(), n18 * 8, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return fail(MS_ERR_HIP, "inverse scale table upload"); }
    owner->d_oscale = d;
    return MS_OK;
}

// ---- the tables of the two-pass coset LDE (lde2_kernels.h) ----------------------------------
// fwd: the CACHED forward plan of the LDE domain; one set per blow-up, built at first use and freed with the plan
int lde2_tables(ms_ntt_plan* fwd, unsigned log_n, unsigned log_b, ms_ntt_plan::Lde2** out) {
    for (auto& l : fwd->lde2) if (l.log_b == log_b) { *out = &l; return MS_OK; }
    const size_t n = (size_t)1 << log_n, L = n >> 8, T = L >> 8, beta = (size_t)1 << log_b;
    const uint64_t wN = gl::root_of_unity(log_n + log_b), wL = gl::root_of_unity(log_n - 8), h = fwd->offset_canon;
    const bool uni = T >= 4;                                      // lde2_kernels.h: uniform split of pass A's factor
    const size_t nt = L >> 6, n_tin = uni ? nt * 256 * 4 : 0, n_tout = uni ? beta * nt * 16 * 4 : 0;
    const size_t T1 = T > 16 ? T / 16 : 0, n_c3 = T1 * 16 * 4;      // pass B, rows of 8192 / 16384 words: w_T^(t1 s0)
    std::vector<uint64_t> host(beta * 256 * 4 + beta * L + 256 * T * 4 + n_tin + n_tout + n_c3);
    uint64_t* gpl = host.data();
    uint64_t* aux = gpl + beta * 256 * 4;
    uint64_t* t2 = aux + beta * L;
    uint64_t* tin4 = t2 + 256 * T * 4;
    uint64_t* tout4 = tin4 + n_tin;
    uint64_t* c3 = tout4 + n_tout;
    const uint64_t sh[4] = {1, (uint64_t)1 << 24, (uint64_t)1 << 48, gl::pow(2, 72)};
    if (uni) {
        const uint64_t wn = gl::root_of_unity(log_n);
        for (size_t i0h = 0; i0h < nt; i0h++) {
            const uint64_t E = 64 * i0h;
            for (size_t b = 0; b < 16; b++) {
                const uint64_t wm = gl::pow(wn, (b * L + E) & (n - 1));          // w_256^b w_n^E
                uint64_t x = 1;
                for (size_t a = 0; a < 16; a++, x = gl::mul(x, wm))
                    for (int c = 0; c < 4; c++) tin4[((i0h * 16 + b) * 16 + a) * 4 + c] = gl::mul(x, sh[c]);
            }
        }
        uint64_t G = h;
        for (size_t j = 0; j < beta; j++, G = gl::mul(G, wN))
            for (size_t i0h = 0; i0h < nt; i0h++) {
                const uint64_t E = 64 * i0h, wm = gl::pow(wn, (16 * E) & (n - 1));
                uint64_t x = gl::pow(G, E);
                for (size_t bp = 0; bp < 16; bp++, x = gl::mul(x, wm))
                    for (int c = 0; c < 4; c++) tout4[((j * nt + i0h) * 16 + bp) * 4 + c] = gl::mul(x, sh[c]);
            }
    }
    uint64_t G = h;                                               // G_j = h w_N^j
    for (size_t j = 0; j < beta; j++, G = gl::mul(G, wN)) {
        const uint64_t GL = gl::pow(G, (uint64_t)L);
        uint64_t x = 1;
        for (size_t i = 0; i < 256; i++) { for (int c = 0; c < 4; c++) gpl[(j * 256 + i) * 4 + c] = gl::mul(x, sh[c]); x = gl::mul(x, GL); }   // plain, 4 copies
        x = 1;
        for (size_t i = 0; i < L; i++) { aux[j * L + i] = gl::to_mont(x); x = gl::mul(x, G); }
    }
    for (size_t k = 0; k < 256; k++) {
        const uint64_t wk = gl::pow(wL, (uint64_t)k);
        uint64_t x = 1;
        for (size_t t = 0; t < T; t++) { for (int c = 0; c < 4; c++) t2[(k * T + t) * 4 + c] = gl::mul(x, sh[c]); x = gl::mul(x, wk); }          // plain, 4 copies
    }
    if (T1) {
        unsigned log_t = 0;
        while (((size_t)1 << log_t) < T) log_t++;
        const uint64_t wT = gl::root_of_unity(log_t);
        for (size_t t1 = 0; t1 < T1; t1++)
            for (size_t s0 = 0; s0 < 16; s0++) {
                const uint64_t x = gl::pow(wT, (uint64_t)(t1 * s0));
                for (int c = 0; c < 4; c++) c3[(t1 * 16 + s0) * 4 + c] = gl::mul(x, sh[c]);
            }
    }
    ms_ntt_plan::Lde2 l;
    l.log_b = log_b;
    if (hipMalloc(&l.d, host.size() * 8) != hipSuccess) return fail(MS_ERR_NOMEM, "LDE tables (%zu bytes)", host.size() * 8);
    if (hipMemcpy(l.d, host.data(), host.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(l.d); return fail(MS_ERR_HIP, "LDE table upload"); }
    l.gpl = l.d; l.aux = l.d + beta * 256 * 4; l.t2 = l.aux + beta * L;
    if (uni) { l.tin4 = l.t2 + 256 * T * 4; l.tout4 = l.tin4 + n_tin; }
    if (T1) l.c3 = l.t2 + 256 * T * 4 + n_tout + n_tin;
    fwd->lde2.push_back(l);
    *out = &fwd->lde2.back();
    return MS_OK;
}
