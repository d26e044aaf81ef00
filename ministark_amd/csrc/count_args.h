// What the entry points of the direct-indexed tables share on the host (ms_range.cpp, ms_bitwise.cpp), from "the records are resolved" on.
//   write_columns   ms_limb_decompose, ms_bitwise_columns: the overlap checks of destinations, read columns and the report, the checked
//                   mode, the [specs | pointer table] upload, the [overflow | active | first] scratch, the writing kernel and its finish
//   count_scratch   ms_range_multiplicities, ms_bitwise_multiplicities: the overlap checks of d_m and d_report, the checked mode, the
//                   MS_*_FORM switch, the [first | missing | cnt[T]] scratch, and the launches the entry point hands in
//   lds_grid        the workgroups of an LDS count
// Each refuses in the order its entry points always have (tests/golden/table_refusals.json).
#pragma once
#include "ms_internal.h"
#include "../../include/ministark_hip_range.h"
#include "direct_count.h"

namespace mscount {

struct Dst { unsigned d0, d1; };              // a spec writes the base columns d0 .. d1 - 1

// what a column writer is, once its specs are resolved.  The last two are where the two entry points have always differed.
template <class Spec>
struct Writer {
    const char *reads_as;                     // "... and column %u, which a spec reads as <reads_as>, overlap"
    const char *clear_scope, *run_scope, *finish_scope;
    void (*run_fp)(msdc::WriterParams<Spec>);
    void (*run_fp252)(msdc::WriterParams<Spec>);
    void (*finish)(msdc::WriterParams<Spec>);
    bool dst_by_address;                      // two specs' destinations clash where their memory does, not only where their indices do
    bool report_with_spec;                    // d_report against a spec's destinations right after that spec's checks, not after all the read columns
};

// R.used: the columns the specs READ.  `bytes`: what the writing kernel moves.
template <class Spec>
static int write_columns(ms_ctx* ctx, const BaseColumns& R, const Writer<Spec>& W, int field, unsigned V, size_t n, void* const* d_base,
                         const std::vector<Spec>& specs, const std::vector<Dst>& dst, void* d_report, double bytes) {
    const char* me = R.me;
    const unsigned nspecs = (unsigned)specs.size();
    const size_t col_bytes = n * V * 8;
    auto report_on = [&](unsigned c) { return ranges_overlap(d_report, sizeof(ms_limb_report), d_base[c], col_bytes); };
    auto report_on_dst = [&](unsigned k) {
        for (unsigned d = dst[k].d0; d < dst[k].d1; d++) if (report_on(d)) return fail(MS_ERR_INVALID, "%s: d_report and base column %u overlap", me, d);
        return (int)MS_OK;
    };
    for (unsigned k = 0; k < nspecs; k++) {
        for (unsigned t = 0; t < k; t++) {
            bool clash = dst[k].d0 < dst[t].d1 && dst[t].d0 < dst[k].d1;
            for (unsigned d = dst[k].d0; W.dst_by_address && d < dst[k].d1; d++)
                for (unsigned e = dst[t].d0; e < dst[t].d1; e++) clash = clash || ranges_overlap(d_base[d], col_bytes, d_base[e], col_bytes);
            if (clash) return fail(MS_ERR_INVALID, "%s: the destination columns of specs %u and %u overlap", me, t, k);
        }
        for (unsigned d = dst[k].d0; d < dst[k].d1; d++)
            for (unsigned c : R.used)
                if (c == d || ranges_overlap(d_base[d], col_bytes, d_base[c], col_bytes))
                    return fail(MS_ERR_INVALID, "%s: spec %u: destination column %u and column %u, which a spec reads as %s, overlap", me, k, d, c, W.reads_as);
        if (W.report_with_spec) MSCHK(report_on_dst(k));
    }
    for (unsigned c : R.used)
        if (report_on(c)) return fail(MS_ERR_INVALID, "%s: d_report and base column %u overlap", me, c);
    for (unsigned k = 0; k < nspecs && !W.report_with_spec; k++) MSCHK(report_on_dst(k));
    if (n && nspecs) MSCHK(canon_named(ctx, me, field, n, (const void* const*)d_base, R.used));      // what the call reads: the destinations may hold anything
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0 || nspecs == 0) {
        HIPCHK(hipMemsetAsync(d_report, 0, sizeof(ms_limb_report), ctx->stream));
        return MS_OK;
    }
    LockedPoolGuard pooled(ctx);
    // [specs | the pointer table] as the kernel reads them; [overflow | active] zero, [first] all ones
    const size_t spec_bytes = nspecs * sizeof(Spec);
    std::vector<char> tab(spec_bytes + (size_t)R.nbase * sizeof(void*));
    memcpy(tab.data(), specs.data(), spec_bytes);
    memcpy(tab.data() + spec_bytes, d_base, (size_t)R.nbase * sizeof(void*));
    const void* d_tab = nullptr;
    MSCHK(stage_view(ctx, tab.data(), tab.size(), &d_tab, pooled));
    void* tmp = nullptr;
    MSCHK(pooled.alloc(24, &tmp));
    msdc::WriterParams<Spec> P;
    memset(&P, 0, sizeof P);
    P.specs = (const Spec*)d_tab; P.base = (uint64_t* const*)((const char*)d_tab + spec_bytes);
    P.overflow = (uint64_t*)tmp; P.active = (uint64_t*)tmp + 1; P.first = (uint64_t*)tmp + 2;
    P.report = (msdc::LimbReport*)d_report; P.n = n;
    { ProfScope ps(ctx, W.clear_scope, 24.0);
      HIPCHK(hipMemsetAsync(tmp, 0, 16, ctx->stream));
      HIPCHK(hipMemsetAsync((char*)tmp + 16, 0xFF, 8, ctx->stream)); }
    const auto run = V == 1 ? W.run_fp : W.run_fp252;
    { ProfScope ps(ctx, W.run_scope, bytes);
      hipLaunchKernelGGL(run, dim3(stream_grid(n), nspecs), dim3(msdc::NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, W.finish_scope, 24.0 + sizeof(ms_limb_report));
      hipLaunchKernelGGL(W.finish, dim3(1), dim3(1), 0, ctx->stream, P); }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// The checks of a count once its sets are resolved (R.used: the columns a set or a mask names), then, under the context's lock, the
// scratch [first | missing | cnt[T]] -- all ones, zero, zero -- written into P with d_m and d_report, and launch(lds): the count and the
// finish.  `form_var`: MS_*_FORM=plain|lds, the counting kernel a probe asks for; otherwise the LDS histogram wherever it exists.
template <class Params, class Launch>
static int count_scratch(ms_ctx* ctx, const BaseColumns& R, int field, unsigned V, size_t n, size_t n_m, void* d_m, void* d_report,
                         const char* form_var, bool has_lds, size_t T, const char* clear_scope, Params& P, Launch launch) {
    const char* me = R.me;
    const size_t col_bytes = n * V * 8, m_bytes = n_m * V * 8;
    for (unsigned c : R.used) {
        if (ranges_overlap(d_m, m_bytes, R.d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_m and base column %u, which a set or a mask names, overlap", me, c);
        if (ranges_overlap(d_report, sizeof(ms_lookup_report), R.d_base[c], col_bytes)) return fail(MS_ERR_INVALID, "%s: d_report and base column %u overlap", me, c);
    }
    if (ranges_overlap(d_m, m_bytes, d_report, sizeof(ms_lookup_report))) return fail(MS_ERR_INVALID, "%s: d_m and d_report overlap", me);
    MSCHK(canon_named(ctx, me, field, n, R.d_base, R.used));          // only what the call reads: d_m may be a column of d_base, of any content
    bool lds = has_lds;                                               // where there is no LDS form, `lds` is the global form
    if (const char* form = getenv(form_var)) {
        if (!strcmp(form, "plain")) lds = false;
        else if (strcmp(form, "lds")) return fail(MS_ERR_INVALID, "%s: %s is plain or lds, not %s", me, form_var, form);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LockedPoolGuard pooled(ctx);
    void* tmp = nullptr;
    const size_t zero_bytes = 8 + 4 * T;
    MSCHK(pooled.alloc(8 + zero_bytes, &tmp));
    P.first = (uint64_t*)tmp; P.missing = (uint64_t*)tmp + 1; P.cnt = (uint32_t*)((uint64_t*)tmp + 2);
    P.m = (uint64_t*)d_m; P.report = (mslk::Report*)d_report;
    P.n = n; P.n_m = n_m;
    { ProfScope ps(ctx, clear_scope, (double)(8 + zero_bytes));
      HIPCHK(hipMemsetAsync(tmp, 0xFF, 8, ctx->stream));
      HIPCHK(hipMemsetAsync((char*)tmp + 8, 0, zero_bytes, ctx->stream)); }
    launch(lds);
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// The x extent G of an LDS count's grid.  Every workgroup ends with one global add per non-zero bin of its histogram, whatever the rows
// were, where the count itself is one LDS add per increment: `flush_cost` is four times the bins that one more workgroup in x brings
// (over all of y).  G is the largest number that keeps the flushes at a quarter of the `adds` counted, at most `cap` -- what the device
// holds at once -- and at most one per LNT rows.
static unsigned lds_grid(size_t n, unsigned long long adds, unsigned long long flush_cost, unsigned cap) {
    unsigned long long g = adds / flush_cost;
    g = std::min<unsigned long long>(g, (n + msdc::LNT - 1) / msdc::LNT);
    return (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(g, cap));
}

}  // namespace mscount
