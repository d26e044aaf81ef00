// A stable multi-column key sort of trace rows and a gather by a device-resident index -- a radix sort whose passes a device-side table
// switches off: include/ministark_hip_sort.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_sort.h"
#include "sort_kernels.h"

static_assert(mssort::MAXK == (int)MS_SORT_MAX_KEYS && mssort::MAXCOLS == (int)MS_PERMUTE_MAX_COLUMNS, "sort_kernels.h and the header disagree");
static_assert(sizeof(mssort::Report) == sizeof(ms_sort_report) && sizeof(ms_sort_report) == 16 && sizeof(ms_sort_key) == 32, "record layouts");
static_assert(sizeof(mssort::PermuteParams) <= 4096, "the gather's arguments travel by value");

// one digit position: histograms per tile, their prefix per digit, the stable scatter
static void sort_pass(ms_ctx* ctx, const mssort::Params& P, uint32_t pos, double moved_bytes) {
    using namespace mssort;
    { ProfScope ps(ctx, "sort_pass_hist", (pos == FLAG_POS ? 1.0 : 8.0) * P.n + 1024.0 * P.ntiles);
      hipLaunchKernelGGL(pass_hist, dim3(P.ntiles), dim3(NT), 0, ctx->stream, P, pos); }
#ifdef MS_EMU
    // The simulator starts every thread of a launch, so the 256 workgroups of a skipped scan would cost it what an executed pass costs; its
    // device memory is the host's, so the flag is read here.  pass_hist and pass_scatter take their skips from the table, as in the product.
    const bool scan = !(pos == FLAG_POS ? P.tab->flag_skip : P.tab->skip[pos]);
#else
    const bool scan = true;
#endif
    if (scan) {
        ProfScope ps(ctx, "sort_pass_scan", 2048.0 * P.ntiles);
        hipLaunchKernelGGL(pass_scan, dim3(256), dim3(scan_threads(P.ntiles)), 0, ctx->stream, P, pos);
    }
    { ProfScope ps(ctx, "sort_pass_scatter", moved_bytes + 1024.0 * P.ntiles);
      hipLaunchKernelGGL(pass_scatter, dim3(P.ntiles), dim3(NT), 0, ctx->stream, P, pos); }
}

template <int V>
static void sort_launch(ms_ctx* ctx, const mssort::Params& P) {
    using namespace mssort;
    const double n = (double)P.n;
    const unsigned grid = stream_grid(P.n);
    // algorithmic bytes of a launch that runs; a skipped one moves nothing
    { ProfScope ps(ctx, "sort_prepare", (16.0 * V * P.nkeys + 4.0 + (P.flag ? 8.0 * V + 1.0 : 0.0)) * n);
      hipLaunchKernelGGL((sort_prepare<V>), dim3(std::min<unsigned>(grid, PREPARE_MAX_GRID)), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "sort_decide", (double)sizeof(Table));
      hipLaunchKernelGGL(sort_decide, dim3(1), dim3(64), 0, ctx->stream, P); }
    if (P.flag) sort_pass(ctx, P, FLAG_POS, 1.0 * n + 8.0 * n);
    for (uint32_t W = 0; W < P.nwords; W++) {
        { ProfScope ps(ctx, "sort_gather", 16.0 * n);
          hipLaunchKernelGGL(sort_gather, dim3(grid), dim3(NT), 0, ctx->stream, P, W); }
        for (uint32_t b = 0; b < 8; b++) sort_pass(ctx, P, W * 8 + b, 24.0 * n);
    }
    { ProfScope ps(ctx, "sort_finish", 8.0 * n);
      hipLaunchKernelGGL(sort_finish, dim3(grid), dim3(NT), 0, ctx->stream, P); }
}

extern "C" int ms_sort_rows(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned nkeys, const void* h_key,
                            void* d_perm, void* d_report) {
    const char* me = "ms_sort_rows";
    if (!ctx || !d_base || !h_key || !d_perm || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: keys are columns of a base trace, over Fp or Fp252, not Fq3", me);
    if (nkeys == 0 || nkeys > (unsigned)MS_SORT_MAX_KEYS) return fail(MS_ERR_INVALID, "%s: a key has 1 .. %d components, not %u", me, MS_SORT_MAX_KEYS, nkeys);
    BaseColumns R(me, d_base, nbase);                                 // R.used: the base columns the key or the mask names
    MSCHK(R.null_check());
    const ms_sort_key& H = *(const ms_sort_key*)h_key;
    mssort::Params P;
    memset(&P, 0, sizeof P);
    for (unsigned k = 0; k < nkeys; k++) MSCHK(R.col(H.cols[k], "key ", &P.cols[k]));
    MSCHK(R.mask(H.mask, H.mask_col, "", &P.mask));
    P.mask_kind = H.mask;
    if (n > ((size_t)1 << 30)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu rows (at most 2^30: an index is 32 bits)", me, n);
    const size_t col_bytes = n * V * 8, perm_bytes = n * 4;
    for (unsigned c : R.used) {
        if (ranges_overlap(d_perm, perm_bytes, d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_perm and base column %u, which the key or the mask names, overlap", me, c);
        if (ranges_overlap(d_report, sizeof(ms_sort_report), d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_report and base column %u overlap", me, c);
    }
    if (ranges_overlap(d_perm, perm_bytes, d_report, sizeof(ms_sort_report))) return fail(MS_ERR_INVALID, "%s: d_perm and d_report overlap", me);
    if (n == 0) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemsetAsync(d_report, 0, sizeof(ms_sort_report), ctx->stream));
        return MS_OK;
    }
    MSCHK(canon_named(ctx, me, field, n, d_base, R.used));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LockedPoolGuard pooled(ctx);
    using namespace mssort;
    P.n = (uint32_t)n; P.nkeys = nkeys; P.nwords = nkeys * V;
    P.ntiles = (uint32_t)((n + TILE - 1) / TILE);
    // [red: count, OR[MAXWORDS] zero | AND[MAXWORDS] ones] [table] [total[256]] [keys[nwords][n]] [kw[2][n]] [perm 1 [n]] [hist[256][ntiles]] [flag[n]]
    const size_t red_bytes = 8 * (1 + 2 * MAXWORDS), tab_bytes = (sizeof(Table) + 7) & ~(size_t)7, total_bytes = 256 * 4;
    const size_t keys_bytes = (size_t)P.nwords * n * 8, kw_bytes = n * 8, perm1_bytes = (perm_bytes + 7) & ~(size_t)7, hist_bytes = (size_t)256 * P.ntiles * 4;
    const bool masked = H.mask != MS_EXT_ALWAYS;
    void* tmp = nullptr;
    MSCHK(pooled.alloc(red_bytes + tab_bytes + total_bytes + keys_bytes + 2 * kw_bytes + perm1_bytes + hist_bytes + (masked ? n : 0), &tmp));
    char* at = (char*)tmp;
    P.red = (uint64_t*)at; at += red_bytes;
    P.tab = (Table*)at; at += tab_bytes;
    P.total = (uint32_t*)at; at += total_bytes;
    P.keys = (uint64_t*)at; at += keys_bytes;
    P.kw[0] = (uint64_t*)at; at += kw_bytes;
    P.kw[1] = (uint64_t*)at; at += kw_bytes;
    P.perm[0] = (uint32_t*)d_perm;
    P.perm[1] = (uint32_t*)at; at += perm1_bytes;
    P.hist = (uint32_t*)at; at += hist_bytes;
    P.flag = masked ? (uint8_t*)at : nullptr;
    P.report = (Report*)d_report;
    { ProfScope ps(ctx, "sort_clear", (double)red_bytes);
      HIPCHK(hipMemsetAsync(P.red, 0, 8 * (1 + MAXWORDS), ctx->stream));
      HIPCHK(hipMemsetAsync(P.red + 1 + MAXWORDS, 0xFF, 8 * MAXWORDS, ctx->stream)); }
    if (V == 1) sort_launch<1>(ctx, P);
    else sort_launch<4>(ctx, P);
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_permute_columns(ms_ctx* ctx, int field, size_t n_src, const void* const* d_src, void* const* d_dst, unsigned ncols,
                                  const void* d_index, size_t n_out) {
    const char* me = "ms_permute_columns";
    if (!ctx || !d_src || !d_dst || !d_index) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (ncols == 0 || ncols > (unsigned)MS_PERMUTE_MAX_COLUMNS) return fail(MS_ERR_INVALID, "%s: 1 .. %d columns, not %u", me, MS_PERMUTE_MAX_COLUMNS, ncols);
    for (unsigned c = 0; c < ncols; c++) if (!d_src[c] || !d_dst[c]) return fail(MS_ERR_INVALID, "%s: null column %u", me, c);
    if (n_src > ((size_t)1 << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu source rows (at most 2^32: an index is 32 bits)", me, n_src);
    const size_t src_bytes = n_src * V * 8, dst_bytes = n_out * V * 8, index_bytes = n_out * 4;
    for (unsigned c = 0; c < ncols; c++) {                            // lanes read any row of any source while others store
        for (unsigned s = 0; s < ncols; s++)
            if (ranges_overlap(d_dst[c], dst_bytes, d_src[s], src_bytes)) return fail(MS_ERR_INVALID, "%s: destination %u and source column %u overlap", me, c, s);
        if (ranges_overlap(d_dst[c], dst_bytes, d_index, index_bytes)) return fail(MS_ERR_INVALID, "%s: destination %u and the index overlap", me, c);
        for (unsigned s = 0; s < c; s++)
            if (ranges_overlap(d_dst[c], dst_bytes, d_dst[s], dst_bytes)) return fail(MS_ERR_INVALID, "%s: destinations %u and %u overlap", me, s, c);
    }
    if (n_out == 0) return MS_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    mssort::PermuteParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < ncols; c++) { P.src[c] = (const uint64_t*)d_src[c]; P.dst[c] = (uint64_t*)d_dst[c]; }
    P.index = (const uint32_t*)d_index; P.n_src = n_src; P.n_out = n_out;
    const dim3 grid(std::max(1u, stream_grid(n_out) / std::min(ncols, 16u)), ncols);
    { ProfScope ps(ctx, "permute_columns", (16.0 * V + 4.0) * n_out * ncols);
      if (V == 1) hipLaunchKernelGGL((mssort::permute_columns<1>), grid, dim3(mssort::NT), 0, ctx->stream, P);
      else if (V == 3) hipLaunchKernelGGL((mssort::permute_columns<3>), grid, dim3(mssort::NT), 0, ctx->stream, P);
      else hipLaunchKernelGGL((mssort::permute_columns<4>), grid, dim3(mssort::NT), 0, ctx->stream, P); }
    HIPCHK(hipGetLastError());
    return MS_OK;
}
