// Deriving a padded table where the trace lies -- select rows, fill clock gaps, pad: include/ministark_hip_gaps.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_gaps.h"
#include "gap_kernels.h"
#include <cstddef>

static_assert(msgap::MAXGROUP == (int)MS_GAP_MAX_GROUP && msgap::MAXCOLS == (int)MS_GAP_MAX_COLUMNS, "gap_kernels.h and the header disagree");
static_assert(msgap::COPY == (int)MS_GAP_COPY && msgap::ZERO == (int)MS_GAP_ZERO && msgap::COUNTER == (int)MS_GAP_COUNTER && msgap::FLAG == (int)MS_GAP_FLAG,
              "gap_kernels.h and the header disagree on the column kinds");
static_assert(sizeof(msgap::Report) == sizeof(ms_gap_report) && sizeof(ms_gap_report) == 64 && sizeof(ms_gap_spec) == 32 && sizeof(ms_gap_column) == 8, "record layouts");
static_assert(offsetof(msgap::Report, first_unordered) == offsetof(ms_gap_report, first_unordered) && offsetof(ms_gap_report, first_unordered) == 40, "record layouts");
static_assert(sizeof(msgap::FillParams) <= 4096, "the fill's arguments travel by value");

extern "C" int ms_gap_plan(ms_ctx* ctx, int field, size_t n_src, const void* const* d_base, unsigned nbase, const void* h_spec, const void* d_perm,
                           size_t n, void* d_start, void* d_report) {
    const char* me = "ms_gap_plan";
    if (!ctx || !d_base || !h_spec || !d_start || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: the columns are those of a base trace, over Fp or Fp252, not Fq3", me);
    BaseColumns R(me, d_base, nbase);                                 // R.used: the base columns the spec names
    MSCHK(R.null_check());
    const ms_gap_spec& H = *(const ms_gap_spec*)h_spec;
    if (H.ngroup < 0 || H.ngroup > (int)MS_GAP_MAX_GROUP) return fail(MS_ERR_INVALID, "%s: a group has 0 .. %d columns, not %d", me, MS_GAP_MAX_GROUP, H.ngroup);
    msgap::PlanParams P;
    memset(&P, 0, sizeof P);
    for (int g = 0; g < H.ngroup; g++) MSCHK(R.col(H.group[g], "group ", &P.group[g]));
    if (H.counter >= 0) MSCHK(R.col(H.counter, "counter ", &P.counter));
    MSCHK(R.mask(H.mask, H.mask_col, "", &P.mask));
    P.mask_kind = H.mask;
    P.ngroup = P.counter ? (uint32_t)H.ngroup : 0u;                   // without a counter no gap is computed: the groups are not read
    if (n > ((size_t)1 << 30)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu positions (at most 2^30)", me, n);
    if (n_src > ((size_t)1 << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu source rows (at most 2^32: an index is 32 bits)", me, n_src);
    const size_t col_bytes = n_src * V * 8, perm_bytes = n * 4, start_bytes = (n + 1) * 8;
    for (unsigned c : R.used) {
        if (ranges_overlap(d_start, start_bytes, d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_start and base column %u, which the spec names, overlap", me, c);
        if (ranges_overlap(d_report, sizeof(ms_gap_report), d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_report and base column %u overlap", me, c);
    }
    if (d_perm && ranges_overlap(d_start, start_bytes, d_perm, perm_bytes)) return fail(MS_ERR_INVALID, "%s: d_start and d_perm overlap", me);
    if (d_perm && ranges_overlap(d_report, sizeof(ms_gap_report), d_perm, perm_bytes)) return fail(MS_ERR_INVALID, "%s: d_report and d_perm overlap", me);
    if (ranges_overlap(d_start, start_bytes, d_report, sizeof(ms_gap_report))) return fail(MS_ERR_INVALID, "%s: d_start and d_report overlap", me);
    if (n) MSCHK(canon_named(ctx, me, field, n_src, d_base, R.used));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    { ProfScope ps(ctx, "gap_clear", (double)sizeof(ms_gap_report));
      HIPCHK(hipMemsetAsync(d_report, 0, sizeof(ms_gap_report), ctx->stream));
      HIPCHK(hipMemsetAsync((char*)d_report + offsetof(ms_gap_report, first_unordered), 0xFF, 8, ctx->stream)); }
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_start, 0, 8, ctx->stream));
        return MS_OK;
    }
    LockedPoolGuard pooled(ctx);
    using namespace msgap;
    P.perm = (const uint32_t*)d_perm; P.start = (uint64_t*)d_start; P.report = (Report*)d_report;
    P.n_src = n_src; P.n = (uint32_t)n; P.ntiles = (uint32_t)((n + TILE - 1) / TILE);
    void* tmp = nullptr;
    MSCHK(pooled.alloc((size_t)P.ntiles * 8, &tmp));
    P.tile_sum = (uint64_t*)tmp;
    const double dn = (double)n;
    { ProfScope ps(ctx, "gap_count", ((P.perm ? 8.0 : 0.0) + 8.0 * V * ((P.counter ? 1.0 : 0.0) + 2.0 * P.ngroup + (P.mask ? 1.0 : 0.0)) + 8.0) * dn);
      if (V == 1) hipLaunchKernelGGL((gap_count<1>), dim3(P.ntiles), dim3(NT), 0, ctx->stream, P);
      else hipLaunchKernelGGL((gap_count<4>), dim3(P.ntiles), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "gap_scan", 16.0 * P.ntiles);
      hipLaunchKernelGGL(gap_scan, dim3(1), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "gap_starts", 16.0 * dn);
      hipLaunchKernelGGL(gap_starts, dim3(P.ntiles), dim3(NT), 0, ctx->stream, P); }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_gap_fill(ms_ctx* ctx, int field, size_t n_src, const void* const* d_base, unsigned nbase, const void* d_perm, size_t n,
                           const void* d_start, const void* h_columns, void* const* d_dst, unsigned ncols, size_t n_out) {
    const char* me = "ms_gap_fill";
    if (!ctx || !d_base || !d_start || !h_columns || !d_dst) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: the columns are those of a base trace, over Fp or Fp252, not Fq3", me);
    if (ncols == 0 || ncols > (unsigned)MS_GAP_MAX_COLUMNS) return fail(MS_ERR_INVALID, "%s: 1 .. %d columns, not %u", me, MS_GAP_MAX_COLUMNS, ncols);
    BaseColumns R(me, d_base, nbase);                                 // R.used: the base columns a record names
    MSCHK(R.null_check());
    const ms_gap_column* H = (const ms_gap_column*)h_columns;
    msgap::FillParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) {
        if (!d_dst[c]) return fail(MS_ERR_INVALID, "%s: null destination %u", me, c);
        if (H[c].kind < MS_GAP_COPY || H[c].kind > MS_GAP_FLAG) return fail(MS_ERR_INVALID, "%s: column %u: unknown kind %d", me, c, H[c].kind);
        P.kind[c] = (uint8_t)H[c].kind;
        P.dst[c] = (uint64_t*)d_dst[c];
        if (H[c].kind == MS_GAP_FLAG) continue;
        char what[32];
        snprintf(what, sizeof what, "column %u: source ", c);
        MSCHK(R.col(H[c].src, what, &P.src[c]));
    }
    if (n > ((size_t)1 << 30)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu positions (at most 2^30)", me, n);
    if (n_out > ((size_t)1 << 30)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu output rows (at most 2^30)", me, n_out);
    if (n_src > ((size_t)1 << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu source rows (at most 2^32: an index is 32 bits)", me, n_src);
    const size_t col_bytes = n_src * V * 8, dst_bytes = n_out * V * 8, perm_bytes = n * 4, start_bytes = (n + 1) * 8;
    for (unsigned c = 0; c < ncols; c++) {                            // lanes read any row of any source while others store
        for (unsigned s : R.used)
            if (ranges_overlap(d_dst[c], dst_bytes, d_base[s], col_bytes)) return fail(MS_ERR_INVALID, "%s: destination %u and base column %u overlap", me, c, s);
        if (d_perm && ranges_overlap(d_dst[c], dst_bytes, d_perm, perm_bytes)) return fail(MS_ERR_INVALID, "%s: destination %u and d_perm overlap", me, c);
        if (ranges_overlap(d_dst[c], dst_bytes, d_start, start_bytes)) return fail(MS_ERR_INVALID, "%s: destination %u and d_start overlap", me, c);
        for (unsigned s = 0; s < c; s++)
            if (ranges_overlap(d_dst[c], dst_bytes, d_dst[s], dst_bytes)) return fail(MS_ERR_INVALID, "%s: destinations %u and %u overlap", me, s, c);
    }
    if (n_out == 0) return MS_OK;
    if (n) MSCHK(canon_named(ctx, me, field, n_src, d_base, R.used));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    using namespace msgap;
    P.perm = (const uint32_t*)d_perm; P.start = (const uint64_t*)d_start; P.n_src = n_src; P.n_out = n_out; P.n = (uint32_t)n;
    const dim3 grid((unsigned)((n_out + OUT_TILE - 1) / OUT_TILE), ncols);
    { ProfScope ps(ctx, "gap_fill", (16.0 * V + 8.0) * n_out * ncols);
      if (V == 1) hipLaunchKernelGGL((gap_fill<1>), grid, dim3(NT), 0, ctx->stream, P);
      else hipLaunchKernelGGL((gap_fill<4>), grid, dim3(NT), 0, ctx->stream, P); }
    HIPCHK(hipGetLastError());
    return MS_OK;
}
