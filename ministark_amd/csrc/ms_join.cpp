// Join rows against a table -- the hash-table build of the lookup layer over a table side of its own, and a probe that writes the row
// it finds: include/ministark_hip_join.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_join.h"
#include "join_kernels.h"

static_assert(mslk::MAXW == (int)MS_JOIN_MAX_WIDTH && mslk::MAXSETS == (int)MS_JOIN_MAX_SETS, "lookup_kernels.h and the header disagree");
static_assert(sizeof(msjn::Report) == sizeof(ms_join_report) && sizeof(ms_join_report) == 48 && sizeof(ms_lookup_tuple) == 32, "record layouts");
static_assert(msjn::NONE == MS_JOIN_NONE && mslk::EMPTY == MS_JOIN_NONE, "an empty slot and an unmatched row are the same word");

template <int V>
static void join_launch(ms_ctx* ctx, const msjn::Params& P, const mslk::Params& B, unsigned nsets) {
    using namespace msjn;
    const double key = 8.0 * V * P.width;
    // algorithmic bytes: what a walk of ONE step moves (longer walks and the atomics' round trips come on top)
    if (P.n_table) {
        const unsigned grid = stream_grid(P.n_table);
        { ProfScope ps(ctx, "join_build", (key + 4.0) * (double)P.n_table);
          hipLaunchKernelGGL((mslk::lookup_build<V>), dim3(grid), dim3(NT), 0, ctx->stream, B); }
        if (P.table.mask_kind != mstab::MASK_ALWAYS) {
            ProfScope ps(ctx, "join_table_active", 8.0 * V * (double)P.n_table);
            hipLaunchKernelGGL((join_table_active<V>), dim3(grid), dim3(NT), 0, ctx->stream, P);
        }
    }
    if (nsets && P.n) {
        ProfScope ps(ctx, "join_match", nsets * (2.0 * key + 8.0) * (double)P.n);       // the key, a slot, the table row's key, the index
        hipLaunchKernelGGL((join_match<V>), dim3(stream_grid(P.n), nsets), dim3(NT), 0, ctx->stream, P);
    }
    { ProfScope ps(ctx, "join_finish", 40.0 + sizeof(Report));
      hipLaunchKernelGGL(join_finish, dim3(1), dim3(1), 0, ctx->stream, P); }
}

extern "C" int ms_join_rows(ms_ctx* ctx, int field, size_t n_table, const void* const* d_table, unsigned ntable_cols, const void* h_table_key,
                            size_t n, const void* const* d_base, unsigned nbase, unsigned width,
                            const void* h_keys, unsigned nsets, void* const* d_match, void* d_report) {
    const char* me = "ms_join_rows";
    if (!ctx || !d_table || !h_table_key || !d_base || (nsets && (!h_keys || !d_match)) || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: keys are rows of base tables, over Fp or Fp252, not Fq3", me);
    if (width == 0 || width > (unsigned)MS_JOIN_MAX_WIDTH) return fail(MS_ERR_INVALID, "%s: a key has 1 .. %d components, not %u", me, MS_JOIN_MAX_WIDTH, width);
    if (nsets > (unsigned)MS_JOIN_MAX_SETS) return fail(MS_ERR_UNSUPPORTED, "%s: %u key sets in one call (at most %d)", me, nsets, MS_JOIN_MAX_SETS);
    for (unsigned s = 0; s < nsets; s++) if (!d_match[s]) return fail(MS_ERR_INVALID, "%s: null d_match[%u]", me, s);
    BaseColumns T(me, d_table, ntable_cols), R(me, d_base, nbase);    // .used: the columns of each side that a key or a mask names
    for (unsigned c = 0; c < ntable_cols; c++) if (!d_table[c]) return fail(MS_ERR_INVALID, "%s: null table column %u", me, c);
    MSCHK(R.null_check());
    msjn::Params P;
    memset(&P, 0, sizeof P);
    {
        const ms_lookup_tuple& H = *(const ms_lookup_tuple*)h_table_key;
        const char* who = "d_table, the table key: ";
        for (unsigned c = 0; c < width; c++) MSCHK(T.col(H.cols[c], who, &P.table.cols[c]));
        MSCHK(T.mask(H.mask, H.mask_col, who, &P.table.mask));
        P.table.mask_kind = H.mask;
    }
    for (unsigned s = 0; s < nsets; s++) {
        const ms_lookup_tuple& H = ((const ms_lookup_tuple*)h_keys)[s];
        char who[40];
        snprintf(who, sizeof who, "d_base, key set %u: ", s);
        for (unsigned c = 0; c < width; c++) MSCHK(R.col(H.cols[c], who, &P.sets[s].cols[c]));
        MSCHK(R.mask(H.mask, H.mask_col, who, &P.sets[s].mask));
        P.sets[s].mask_kind = H.mask;
        P.match[s] = (uint32_t*)d_match[s];
    }
    if (n_table > ((size_t)1 << 30)) return fail(MS_ERR_UNSUPPORTED, "%s: a table of %zu rows (at most 2^30: a slot is a 32-bit row index)", me, n_table);
    if (n > ((size_t)1 << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu rows (at most 2^32: the first missing row travels as set << 32 | row)", me, n);
    const size_t tcol_bytes = n_table * V * 8, col_bytes = n * V * 8, match_bytes = n * 4;
    // an output against every column that is read, on either side
    auto reads = [&](const void* out, size_t bytes, const char* what, int s) -> int {
        for (unsigned c : T.used)
            if (ranges_overlap(out, bytes, d_table[c], tcol_bytes)) return s < 0 ? fail(MS_ERR_INVALID, "%s: %s and table column %u, which the key or its mask names, overlap", me, what, c)
                                                                                 : fail(MS_ERR_INVALID, "%s: %s[%d] and table column %u, which the key or its mask names, overlap", me, what, s, c);
        for (unsigned c : R.used)
            if (ranges_overlap(out, bytes, d_base[c], col_bytes)) return s < 0 ? fail(MS_ERR_INVALID, "%s: %s and base column %u, which a key or a mask names, overlap", me, what, c)
                                                                               : fail(MS_ERR_INVALID, "%s: %s[%d] and base column %u, which a key or a mask names, overlap", me, what, s, c);
        return MS_OK;
    };
    MSCHK(reads(d_report, sizeof(ms_join_report), "d_report", -1));
    for (unsigned s = 0; s < nsets; s++) {
        MSCHK(reads(d_match[s], match_bytes, "d_match", (int)s));
        if (ranges_overlap(d_match[s], match_bytes, d_report, sizeof(ms_join_report))) return fail(MS_ERR_INVALID, "%s: d_match[%u] and d_report overlap", me, s);
        for (unsigned t = 0; t < s; t++)
            if (ranges_overlap(d_match[s], match_bytes, d_match[t], match_bytes)) return fail(MS_ERR_INVALID, "%s: d_match[%u] and d_match[%u] overlap", me, t, s);
    }
    MSCHK(canon_named(ctx, me, field, n_table, d_table, T.used, "d_table"));
    if (nsets) MSCHK(canon_named(ctx, me, field, n, d_base, R.used));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LockedPoolGuard pooled(ctx);
    size_t cap = 2;                                                   // sized by the TABLE: a small one stays in cache whatever is joined against it
    while (cap < 2 * n_table) cap <<= 1;
    // [first | slots[cap]] all ones, [matched | missing | dups | tact] zero
    void* tmp = nullptr;
    const size_t ones_bytes = 8 + cap * 4, zero_bytes = 32;
    MSCHK(pooled.alloc(ones_bytes + zero_bytes, &tmp));
    uint64_t* zeros = (uint64_t*)((char*)tmp + ones_bytes);           // cap is even: 8-byte aligned
    P.first = (uint64_t*)tmp; P.slots = (const uint32_t*)((char*)tmp + 8);
    P.matched = zeros; P.missing = zeros + 1; P.dups = zeros + 2; P.tact = zeros + 3;
    P.report = (msjn::Report*)d_report;
    P.n_table = n_table; P.n = n; P.capmask = (uint32_t)(cap - 1); P.width = width;
    mslk::Params B;                                                   // what lookup_build reads: table, n, slots, capmask, width, dups
    memset(&B, 0, sizeof B);
    B.table = P.table; B.n = n_table; B.slots = (uint32_t*)((char*)tmp + 8); B.capmask = P.capmask; B.width = width; B.dups = P.dups;
    { ProfScope ps(ctx, "join_clear", (double)(ones_bytes + zero_bytes));
      HIPCHK(hipMemsetAsync(tmp, 0xFF, ones_bytes, ctx->stream));
      HIPCHK(hipMemsetAsync(zeros, 0, zero_bytes, ctx->stream)); }
    if (V == 1) join_launch<1>(ctx, P, B, nsets);
    else join_launch<4>(ctx, P, B, nsets);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
