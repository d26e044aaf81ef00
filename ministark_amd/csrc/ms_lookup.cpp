// The multiplicity column of a LogUp lookup -- a hash-table build and probe over device atomics: include/ministark_hip_lookup.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_lookup.h"
#include "lookup_kernels.h"

static_assert(mslk::MAXW == (int)MS_LOOKUP_MAX_WIDTH && mslk::MAXSETS == (int)MS_LOOKUP_MAX_SETS, "lookup_kernels.h and the header disagree");
static_assert(sizeof(mslk::Report) == sizeof(ms_lookup_report) && sizeof(ms_lookup_report) == 32 && sizeof(ms_lookup_tuple) == 32, "record layouts");

template <int V, class F>
static void lookup_launch(ms_ctx* ctx, const mslk::Params& P, unsigned nsets, double key_bytes) {
    using namespace mslk;
    const unsigned grid = stream_grid(P.n);
    const double n = (double)P.n;
    // algorithmic bytes: what a walk of ONE step moves (longer walks and the atomics' round trips come on top)
    { ProfScope ps(ctx, "lookup_build", key_bytes + 4.0 * n);
      hipLaunchKernelGGL((lookup_build<V>), dim3(grid), dim3(NT), 0, ctx->stream, P); }
    if (nsets) {
        ProfScope ps(ctx, "lookup_count", nsets * (2.0 * key_bytes + 8.0 * n));       // the key, a slot, the table row's key, the counter
        // MS_LOOKUP_PLAIN_ADDS=1: one atomicAdd per lookup row, the form scripts/lookup_probe.py measures the wave-level one against
        const char* plain = getenv("MS_LOOKUP_PLAIN_ADDS");
        if (plain && plain[0] == '1') hipLaunchKernelGGL((lookup_count<V, false>), dim3(grid, nsets), dim3(NT), 0, ctx->stream, P);
        else hipLaunchKernelGGL((lookup_count<V, true>), dim3(grid, nsets), dim3(NT), 0, ctx->stream, P);
    }
    { ProfScope ps(ctx, "lookup_finish", (4.0 + 8.0 * V) * n);
      hipLaunchKernelGGL((lookup_finish<F>), dim3(grid), dim3(NT), 0, ctx->stream, P); }
}

extern "C" int ms_lookup_multiplicities(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned width,
                                        const void* h_table, const void* h_lookups, unsigned nsets, void* d_m, void* d_report) {
    const char* me = "ms_lookup_multiplicities";
    if (!ctx || !d_base || !h_table || (nsets && !h_lookups) || !d_m || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: tuples are rows of a base trace, over Fp or Fp252, not Fq3", me);
    if (width == 0 || width > (unsigned)MS_LOOKUP_MAX_WIDTH) return fail(MS_ERR_INVALID, "%s: a tuple has 1 .. %d components, not %u", me, MS_LOOKUP_MAX_WIDTH, width);
    if (nsets > (unsigned)MS_LOOKUP_MAX_SETS) return fail(MS_ERR_UNSUPPORTED, "%s: %u lookup sets in one call (at most %d)", me, nsets, MS_LOOKUP_MAX_SETS);
    BaseColumns R(me, d_base, nbase);                                 // R.used: the base columns a tuple or a mask names
    MSCHK(R.null_check());
    mslk::Params P;
    memset(&P, 0, sizeof P);
    for (unsigned s = 0; s <= nsets; s++) {                           // the table, then the sets
        const ms_lookup_tuple& H = s ? ((const ms_lookup_tuple*)h_lookups)[s - 1] : *(const ms_lookup_tuple*)h_table;
        mslk::Tuple& T = s ? P.sets[s - 1] : P.table;
        char who[32];
        if (s) snprintf(who, sizeof who, "lookup set %u: ", s - 1); else snprintf(who, sizeof who, "the table: ");
        for (unsigned c = 0; c < width; c++) MSCHK(R.col(H.cols[c], who, &T.cols[c]));
        MSCHK(R.mask(H.mask, H.mask_col, who, &T.mask));
        T.mask_kind = H.mask;
    }
    if (n > ((size_t)1 << 30)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu rows (at most 2^30: a slot is a 32-bit row index)", me, n);
    if ((unsigned long long)nsets * n >= (1ull << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %u sets of %zu rows (the counters are 32-bit: sets * rows < 2^32)", me, nsets, n);
    const size_t col_bytes = n * V * 8;
    for (unsigned c : R.used) {
        if (ranges_overlap(d_m, col_bytes, d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_m and base column %u, which a tuple or a mask names, overlap", me, c);
        if (ranges_overlap(d_report, sizeof(ms_lookup_report), d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_report and base column %u overlap", me, c);
    }
    if (ranges_overlap(d_m, col_bytes, d_report, sizeof(ms_lookup_report))) return fail(MS_ERR_INVALID, "%s: d_m and d_report overlap", me);
    if (n == 0) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemsetAsync(d_report, 0, sizeof(ms_lookup_report), ctx->stream));
        return MS_OK;
    }
    MSCHK(canon_named(ctx, me, field, n, d_base, R.used));            // only what the call reads: d_m may be a column of d_base, of any content
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LockedPoolGuard pooled(ctx);
    size_t cap = 2;
    while (cap < 2 * n) cap <<= 1;
    // [first | slots[cap]] all ones, [missing | dups | cnt[n]] zero
    void* tmp = nullptr;
    const size_t ones_bytes = 8 + cap * 4, zero_bytes = 16 + n * 4;
    MSCHK(pooled.alloc(ones_bytes + zero_bytes + 8, &tmp));
    char* zeros = (char*)tmp + ((ones_bytes + 7) & ~(size_t)7);
    P.first = (uint64_t*)tmp; P.slots = (uint32_t*)((char*)tmp + 8);
    P.missing = (uint64_t*)zeros; P.dups = (uint64_t*)zeros + 1; P.cnt = (uint32_t*)(zeros + 16);
    P.m = (uint64_t*)d_m; P.report = (mslk::Report*)d_report;
    P.n = n; P.capmask = (uint32_t)(cap - 1); P.width = width;
    { ProfScope ps(ctx, "lookup_clear", (double)(ones_bytes + zero_bytes));
      HIPCHK(hipMemsetAsync(tmp, 0xFF, ones_bytes, ctx->stream));
      HIPCHK(hipMemsetAsync(zeros, 0, zero_bytes, ctx->stream)); }
    const double key_bytes = 8.0 * n * V * width;
    if (V == 1) lookup_launch<1, msstage::FpT>(ctx, P, nsets, key_bytes);
    else lookup_launch<4, msstage::Fp252T>(ctx, P, nsets, key_bytes);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
