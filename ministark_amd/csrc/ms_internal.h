// Internal declarations shared by the translation units of libministark_hip.so (ms_core / ms_ntt_plan / ms_ntt / ms_ntt252 / ms_stage / ms_hash / ms_eval / ms_deep /
// ms_comm / ms_validate / ms_blake2s / ms_canon / ms_coin / ms_keccak / ms_ext / ms_logup / ms_rpo_coin / ms_lookup / ms_sort / ms_gaps / ms_join / ms_poseidon / ms_blake3 / ms_range / ms_bitwise .cpp,
// the SOURCES of build.py): the context, the plan object and what the three NTT units share, error plumbing, the coset-offset decoders, pooled
// scratch, the checked mode's scans and the base-column arguments of the trace-table entry points.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ministark_hip.h"
#include "../../include/ministark_hip_transcript.h"
#include "gl.h"
#include "fp252.h"
#include "ntt_kernels.h"

using msntt::MAXC;

int fail(int code, const char* fmt, ...);
int field_words(int field, unsigned* V);
#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(MS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define MSCHK(expr)                \
    do {                           \
        int r_ = (expr);           \
        if (r_ != MS_OK) return r_; \
    } while (0)
// Byte ranges [a, a + na) and [b, b + nb) of device memory, as fri_fold_impl compares them (an empty range overlaps nothing).  The entry points
// that refuse overlapping buffers (ms_stage.cpp, ms_deep.cpp) check with this before anything is enqueued.
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *p = (const char*)a, *q = (const char*)b;
    return p < q + nb && q < p + na;
}

// The coset offset an entry point takes, one decoder per field: a null pointer is `dflt`, zero is refused ("<what> offset must be ...").
// Goldilocks: the Montgomery word in, the canonical residue out.  252-bit field: Montgomery limbs in and out, refused unless canonical too.
static inline int offset_gl(const void* h_offset, uint64_t* h, uint64_t dflt = 1, const char* what = "coset") {
    *h = dflt;
    if (h_offset) { uint64_t h_m; memcpy(&h_m, h_offset, 8); *h = gl::from_mont(h_m); }
    if (*h == 0) return fail(MS_ERR_INVALID, "%s offset must be non-zero", what);
    return MS_OK;
}
static inline int offset252(const void* h_offset, f252::E* h, const f252::E& dflt = f252::one(), const char* what = "coset") {
    *h = dflt;
    if (h_offset) memcpy(h->l, h_offset, 32);
    if (f252::is_zero(*h) || f252::geq_p(*h)) return fail(MS_ERR_INVALID, "%s offset must be a non-zero canonical element", what);
    return MS_OK;
}

// what the specialised constraint kernels cost and where they came from (eval_jit.h, jit_cache.h; ms_eval_jit_stats)
struct JitStats { uint64_t compiled = 0, from_disk = 0, failures = 0, damaged_entries = 0; double compile_ms = 0, load_ms = 0; };
JitStats& jit_process_stats();              // the process-wide totals (ms_eval_jit_check has no context)

struct ms_ntt_plan;
static constexpr int MAX_CHAINS = 4;
struct PlanKey { unsigned V, log_n; bool inverse; uint64_t h; };
struct ms_ctx {
    int device = 0;
    std::vector<std::pair<PlanKey, ms_ntt_plan*>> plan_cache;   // plans used by the fused entry points
    hipStream_t stream = nullptr;
    // side streams of run_passes, between a fork and a join event each (ctx_side_streams creates them on first use): the second half of a
    // column group under MS_NTT_STREAMS=2, chains 1 .. S-1 of the column chains.  MAX_CHAINS streams with ctx->stream: the runtime's queue limit
    hipStream_t side[MAX_CHAINS - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[MAX_CHAINS - 1] = {};
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    // columns are processed in groups of about this size (= the scratch buffer).  Measured at 2^24: one column per
    // launch (4096 tiles = exactly two rounds of resident workgroups) loses 5 % of kernel time to the launch tail
    // against 8 columns per launch; the passes are VALU-bound, so there is no cache-locality argument for small groups.
    size_t group_bytes = (size_t)1 << 30;
    std::mutex mu;
    // freed device blocks, by size: GpuVec churn (clone / resize in src/matrix.rs:155-208, the LdeCache of
    // src/eval_gpu.rs:857-898) must not cost a hipMalloc + hipFree pair per column.  All work is ordered on
    // one stream, so a block can be handed out again without synchronising.
    std::multimap<size_t, void*> pool;
    size_t pool_bytes = 0, pool_cap = (size_t)96 << 30;
    std::map<void*, size_t> live;            // size of every block handed out by ms_alloc
    // The public coins created on this context, all three families in one registry keyed by the device state (coin_host.h).  `family` keeps one family's entry points from
    // taking another's handles, `hash` is the byte coin's MS_HASH_*, n_draws mirrors a Poseidon coin's counter (ms_hades_coin.cpp): a draw past 2^64 is refused without a host wait.
    struct CoinRec { int family, hash; uint64_t n_draws; };
    std::map<void*, CoinRec> coins;
    // pinned staging ring for the small host arrays entry points take (query positions, digest indices): the copy to the
    // device is then truly asynchronous and the call does not drain the stream (stage_upload)
    char* stage = nullptr;
    size_t stage_bytes = 0, stage_off = 0;
    // pinned landing buffer of the small downloads (roots, out-of-domain values, the gathers of an opening): a copy into pinned memory
    // + memcpy is 12 us where the same copy into the caller's pageable buffer is 20 us (scripts/download_latency.hip)
    char* land = nullptr;
    std::mutex land_mu;
    void* comm = nullptr;                    // ncclComm_t once ms_comm_init has run
    int comm_rank = 0, comm_size = 1;
    void* prog_buf = nullptr;                // device copy of the current constraint program + constants
    size_t prog_bytes = 0;
    // constraint programs compiled to specialised kernels (eval_jit.h), by hash of the generated source;
    // nullptr = compilation failed once, use the interpreter
    std::map<std::string, hipFunction_t> jit_cache;   // keyed by the full source text, not a hash of it
    std::vector<hipModule_t> jit_modules;
    JitStats jit_stats;
    // optional per-launch timing (ms_profile_*): hipEvent pairs around every kernel launch
    bool profiling = false;
    // checked mode (ms_ctx_set_checked; MS_CHECK_CANONICAL=1 at ms_ctx_create): every entry point that does arithmetic on field data scans
    // its inputs for non-canonical elements first (ms_canon.cpp) and refuses before anything is enqueued
    bool checked = false;
    struct ProfRec { const char* name; hipEvent_t e0, e1; double bytes; };
    std::vector<ProfRec> prof;
};

// RAII: brackets one kernel launch with events on the context's stream when profiling is on
struct ProfScope {
    ms_ctx* ctx; hipEvent_t e0 = nullptr, e1 = nullptr; const char* name; double bytes;
    ProfScope(ms_ctx* c, const char* nm, double algorithmic_bytes) : ctx(c), name(nm), bytes(algorithmic_bytes) {
        if (!ctx->profiling) return;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, ctx->stream);
    }
    ~ProfScope() {
        if (!ctx->profiling) return;
        (void)hipEventRecord(e1, ctx->stream);
        ctx->prof.push_back({name, e0, e1, bytes});
    }
};


int ctx_scratch(ms_ctx* ctx, size_t bytes, void** out);
int ctx_side_streams(ms_ctx* ctx, unsigned count);                // side[0 .. count) and their events exist afterwards; the caller holds ctx->mu
void ctx_side_sync(ms_ctx* ctx);                                  // waits for whatever the side streams still hold
int pool_alloc(ms_ctx* ctx, size_t bytes, void** d_ptr);          // the caller holds ctx->mu
int pool_free(ms_ctx* ctx, void* d_ptr);
int stage_upload(ms_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);   // the caller holds ctx->mu; h_src may be reused at once
// Pooled temporaries of an entry point, returned to the pool on EVERY exit path (an early return through
// MSCHK / HIPCHK used to strand them in ctx->live until ms_ctx_destroy).  PoolGuard goes through the locking
// public calls and must outlive the function's lock scope; LockedPoolGuard is for code that already holds
// ctx->mu and must be declared after the lock_guard (so that it is destroyed first).
struct PoolGuard {
    ms_ctx* ctx; std::vector<void*> blocks;
    explicit PoolGuard(ms_ctx* c) : ctx(c) {}
    int alloc(size_t bytes, void** p) { const int rc = ms_alloc(ctx, bytes, p); if (rc == MS_OK) blocks.push_back(*p); return rc; }
    ~PoolGuard() { for (void* b : blocks) (void)ms_free(ctx, b); }
    PoolGuard(const PoolGuard&) = delete; PoolGuard& operator=(const PoolGuard&) = delete;
};
struct LockedPoolGuard {
    ms_ctx* ctx; std::vector<void*> blocks;
    explicit LockedPoolGuard(ms_ctx* c) : ctx(c) {}
    int alloc(size_t bytes, void** p) { const int rc = pool_alloc(ctx, bytes, p); if (rc == MS_OK) blocks.push_back(*p); return rc; }
    ~LockedPoolGuard() { for (void* b : blocks) (void)pool_free(ctx, b); }
    LockedPoolGuard(const LockedPoolGuard&) = delete; LockedPoolGuard& operator=(const LockedPoolGuard&) = delete;
};

int stage_view(ms_ctx* ctx, const void* h_src, size_t bytes, const void** d_view, LockedPoolGuard& pooled);   // the caller holds ctx->mu

struct ms_ntt_plan {
    ms_ctx* ctx = nullptr;
    // ms_ntt_plan_create hands out a HANDLE: a copy of the context's cached plan for (field, size, direction, offset)
    // with its own queue; `base` is that cached plan (owner of every table), `refs` counts the handles on a cached plan
    // (the cache never evicts a plan in use).  Building the tables of a 2^22-point plan on the host and uploading them
    // cost 1.3 ms per GpuFft / GpuIfft object -- 2.7 ms of the 16.7 ms prover run -- before plans were shared.
    ms_ntt_plan* base = nullptr;
    int refs = 0;
    unsigned V = 1, log_n = 0;
    bool inverse = false, coset = false;
    // small path (log_n < 12)
    bool small = false;
    bool tiny_fused = false;            // Fp, 2^9 .. 2^11 points: the tables of the (256, n / 256) plan are there too (ntt_fused_tiny)
    uint64_t *d_tw = nullptr, *d_scale_in = nullptr, *d_scale_out = nullptr;
    // multi-pass path
    int npass = 0;
    unsigned lr[4] = {0, 0, 0, 0};      // log2 radix per pass
    unsigned log_s[4] = {0, 0, 0, 0};   // log2 element stride of the pass's digit
    unsigned nfields[4] = {0, 0, 0, 0};
    msntt::DigitField fields[4][3];
    unsigned lo_bits = 0;
    uint64_t *d_tw_lo = nullptr, *d_tw_hi = nullptr, *d_aux_lo = nullptr, *d_aux_hi = nullptr, *d_gtab = nullptr;
    uint64_t* d_wr[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t scale_const = 0;
    int scale_mode = 0;                 // last pass: 0 none, 1 const, 2 table
    uint64_t* d_tables = nullptr;       // one allocation backing every table
    // limb-form passes (ntt2_kernels.h): plain tables of 4 pre-shifted copies per twiddle
    uint64_t* d_wr4[4] = {nullptr, nullptr, nullptr, nullptr};    // radix-256 passes: w_256^e
    uint64_t* d_twu4[4] = {nullptr, nullptr, nullptr, nullptr};   // middle passes: per-tile factor [U][k]
    uint64_t *d_sc4 = nullptr, *d_g4 = nullptr, *d_scu4 = nullptr;
    // three-pass plans (last radix 256 since round 3): pass 1's inter-pass factor from wave-uniform tables, the per-lane
    // remainder applied by pass 2 on its loads (ntt2_first_pass<.., UNI>, ntt2_mid_pass<.., LOADQ>)
    bool uni = false;
    uint64_t *d_tin4 = nullptr, *d_tout4 = nullptr;
    uint64_t* d_lq = nullptr;            // pass 2 of such a plan with V = 1 and middle radix 256: the per-lane factor, one plain word per (block, k1)
    // two-pass coset LDE (lde2_kernels.h), built on first use on the forward plan of the LDE domain: per blow-up
    // [gpl | aux | t2] in one allocation
    struct Lde2 { unsigned log_b = 0; uint64_t *d = nullptr, *gpl = nullptr, *aux = nullptr, *t2 = nullptr, *tin4 = nullptr, *tout4 = nullptr, *c3 = nullptr; };
    std::vector<Lde2> lde2;
    uint64_t* d_oscale = nullptr;       // inverse plans of 2^18 points: n^-1 h^-k, k < n (Montgomery), for the two-pass route (built at first use)
    uint64_t offset_canon = 1;          // the coset offset h (canonical)
    std::vector<void*> queue;
    // Fp252 path (V == 4): plain radix-2 plan, see fp252_kernels.h
    bool is252 = false;
    uint64_t *d252_tw_lo = nullptr, *d252_tw_hi = nullptr, *d252_sc_lo = nullptr, *d252_sc_hi = nullptr;
    int scale_in252 = 0, scale_out252 = 0;
    uint64_t off252[4] = {0, 0, 0, 0};  // the coset offset itself: cache lookups compare it, not just its hash
    // tiled passes of fp252_ntt_kernels.h (2^11 <= n <= 2^30): number of passes (0 = radix-2 sequence only), digit sizes,
    // per-pass tables w_R^e (e < R/2)
    int np252 = 0;
    unsigned lr252[3] = {0, 0, 0};
    uint64_t* d252_twr[3] = {nullptr, nullptr, nullptr};
};


// ms_canon.cpp: the checks of the checked mode.  Called WITHOUT ctx->mu, after the entry point's own argument checks and before anything is
// enqueued; MS_OK at once when the mode is off.  `arg` is the argument's name as include/ministark_hip.h spells it.
int canon_cols(ms_ctx* ctx, const char* entry, const char* arg, int field, size_t n, const void* const* d_cols, unsigned ncols);
int canon_col(ms_ctx* ctx, const char* entry, const char* arg, int field, size_t n, const void* d_col);
int canon_rows(ms_ctx* ctx, const char* entry, const char* arg, int field, size_t nrows, unsigned ncols, const void* d_matrix);   // row-major matrix
int canon_host(ms_ctx* ctx, const char* entry, const char* arg, int field, const void* h_elems, size_t count);
int canon_program(ms_ctx* ctx, const char* entry, bool is252, const uint32_t* h_prog, unsigned ninstr, const void* h_consts, unsigned nconst_words,
                  unsigned log_n, const void* h_domain_offset, const void* d_x_lde, const void* const* d_base_cols, unsigned nbase,
                  const void* const* d_ext_cols, unsigned next, const void* const* d_periodic, const unsigned* periodic_len, unsigned nperiodic);
static inline int field_of_words(unsigned V) { return V == 1 ? MS_GOLDILOCKS_FP : V == 3 ? MS_GOLDILOCKS_FQ3 : MS_STARK252_FP; }
// d_base[c] for c in `used` alone (what a call NAMES; the rest of d_base may hold anything); the refusal reports the caller's own column index
int canon_named(ms_ctx* ctx, const char* entry, int field, size_t n, const void* const* d_base, const std::vector<unsigned>& used, const char* arg = "d_base");

// ms_core.cpp: the base-column table (d_base, nbase) of a trace-table entry point (ms_ext / ms_logup / ms_lookup / ms_sort / ms_gaps / ms_join / ms_range / ms_bitwise .cpp):
// resolves the column indices of the caller's records to addresses, refuses the ones out of range, and keeps the list of the columns
// named, in the order first named -- what the overlap checks and canon_named go through.  `what` / `who` open the refusal after
// "<entry>: " and end in a space or in ": " ("key ", "lookup set 1: ", "column 3: term ").
struct BaseColumns {
    const char* me; const void* const* d_base; unsigned nbase;
    std::vector<unsigned> used;
    BaseColumns(const char* entry, const void* const* base, unsigned n) : me(entry), d_base(base), nbase(n) {}
    int null_check() const;                                                     // "null base column %u"
    int col(int index, const char* what, const uint64_t** ptr);                // "<what>column %d out of range (%u)"
    // the mask words of a record: *ptr is null for MS_EXT_ALWAYS, whose mask_col is not looked at
    int mask(int kind, int mask_col, const char* who, const uint64_t** ptr);   // "<who>unknown mask kind %d", "<who>mask column %d out of range (%u)"
};

// ms_ntt_plan.cpp: plans and their tables (host only).  ctx_plan / plan252_cached / plan_oscale / lde2_tables: the caller holds ctx->mu.
// (MS_LOCAL: what the split of ms_ntt.cpp made cross-unit stays out of the library's dynamic symbol table, which is as it was.)
#define MS_LOCAL __attribute__((visibility("hidden")))
int ctx_plan(ms_ctx* ctx, unsigned V, unsigned log_n, bool inverse, uint64_t h, ms_ntt_plan** out);     // the context's cached plan
int plan252_cached(ms_ctx* ctx, unsigned log_n, bool inverse, const f252::E& h, ms_ntt_plan** out);    // h: as offset252 returns it
MS_LOCAL bool user_plan_alive(ms_ntt_plan* p);                // a plan of ms_ntt_plan_create whose context still exists
void plans_release_ctx(ms_ctx* ctx);                 // ms_ctx_destroy: plans still held by the caller go with their context
int plan_free_cached(ms_ntt_plan* plan);             // the context's own (cached) plans
MS_LOCAL int plan_oscale(ms_ntt_plan* owner);                 // d_oscale of a cached inverse coset plan of 2^18 points, built at first use
MS_LOCAL int lde2_tables(ms_ntt_plan* fwd, unsigned log_n, unsigned log_b, ms_ntt_plan::Lde2** out);   // of the cached forward plan, per blow-up
constexpr unsigned NTT252_TILE_LOG = 11;             // = ms252::TILE_LOG (ms_ntt252.cpp asserts it): plans from this size on carry tiled passes
// ms_ntt252.cpp: the 252-bit field's transforms
MS_LOCAL int plan_run252(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols);
MS_LOCAL int plan_run252_tiled(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols, unsigned log_zero_ext, bool bitrev_out);
// ms_ntt.cpp: the Goldilocks routes (plan_run hands a 252-bit plan on), bit reversal
int plan_run(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols, unsigned valid_rows, bool bitrev_out = false);
int bit_reverse_run(ms_ctx* ctx, unsigned V, unsigned log_n, const void* const* src, void* const* dst, unsigned ncols);
unsigned stream_grid(size_t n);                      // ms_stage.cpp: the grid of a grid-stride kernel over n elements
