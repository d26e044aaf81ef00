// Extension columns between the two trace commitments (Trace::build_extension_columns, src/trace.rs;
// examples/brainfuck/trace.rs:108-289): include/ministark_hip_ext.h.
#include "ext_args.h"

static_assert(msext::MAXTERMS == (int)MS_EXT_MAX_TERMS && msext::MAXEXT == (int)MS_EXT_MAX_COLUMNS, "ext_kernels.h and the header disagree");
static_assert((int)msext::INIT_ZERO == (int)MS_EXT_INIT_ZERO && (int)msext::INIT_ONE == (int)MS_EXT_INIT_ONE && (int)msext::INIT_CHALLENGE == (int)MS_EXT_INIT_CHALLENGE,
              "ext_kernels.h and the header disagree");
// the one place that ties the mask kinds of every trace-table kernel (table_common.h) to the header's: ms_logup / ms_lookup / ms_sort / ms_gaps
// .cpp take MS_EXT_* from the same header and hand the value through
static_assert(mstab::MASK_ALWAYS == (int)MS_EXT_ALWAYS && mstab::MASK_IF_NONZERO == (int)MS_EXT_IF_NONZERO && mstab::MASK_IF_ZERO == (int)MS_EXT_IF_ZERO,
              "table_common.h and the extension header disagree");

template <class F, class B>
static void ext_launch(ms_ctx* ctx, const msext::Params& P, unsigned next, double term_bytes) {
    using namespace msext;
    { ProfScope ps(ctx, "ext_reduce", term_bytes);
      hipLaunchKernelGGL((ext_reduce<F, B>), dim3(P.nblocks, next), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "ext_blocks", 0.0);
      hipLaunchKernelGGL((ext_blocks<F>), dim3(next), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "ext_apply", term_bytes + 8.0 * P.n * F::V * next);
      hipLaunchKernelGGL((ext_apply<F, B>), dim3(P.nblocks, next), dim3(NT), 0, ctx->stream, P); }
}

extern "C" int ms_build_extension_columns(ms_ctx* ctx, int base_field, int ext_field, size_t n, const void* const* d_base, unsigned nbase,
                                          const void* d_challenges, unsigned nchallenges, const void* h_columns, const void* h_terms, unsigned next,
                                          void* const* d_out) {
    const char* me = "ms_build_extension_columns";
    if (!ctx || (nbase && !d_base) || (nchallenges && !d_challenges) || (next && (!h_columns || !d_out))) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned VB = 0, VE = 0;
    if (field_words(base_field, &VB) != MS_OK || field_words(ext_field, &VE) != MS_OK || VB == 3 || (VB == 4) != (VE == 4))
        return fail(MS_ERR_INVALID, "%s: the field pair (base %d, extension %d) is not one of Fp -> Fq3, Fp -> Fp, Fp252 -> Fp252", me, base_field, ext_field);
    if (next > (unsigned)MS_EXT_MAX_COLUMNS) return fail(MS_ERR_UNSUPPORTED, "%s: %u columns in one call (at most %d)", me, next, MS_EXT_MAX_COLUMNS);
    const ms_ext_column* hc = (const ms_ext_column*)h_columns;
    const ms_ext_term* ht = (const ms_ext_term*)h_terms;
    size_t nterms = 0;
    for (unsigned e = 0; e < next; e++) {
        if (hc[e].na > (unsigned)MS_EXT_MAX_TERMS || hc[e].nb > (unsigned)MS_EXT_MAX_TERMS)
            return fail(MS_ERR_UNSUPPORTED, "%s: column %u has %u + %u terms (at most %d per map)", me, e, hc[e].na, hc[e].nb, MS_EXT_MAX_TERMS);
        nterms += hc[e].na + hc[e].nb;
    }
    if (nterms && !ht) return fail(MS_ERR_INVALID, "%s: null argument", me);
    BaseColumns R(me, d_base, nbase);
    MSCHK(R.null_check());
    std::vector<msext::Column> cols(next);
    size_t at = 0;
    double term_bytes = 0;
    for (unsigned e = 0; e < next; e++) {
        const ms_ext_column& H = hc[e];
        msext::Column& C = cols[e];
        memset(&C, 0, sizeof C);
        MSCHK(msextargs::column_header(R, e, H, nchallenges, d_out[e], n, VB, &C, &term_bytes));
        C.na = H.na; C.nb = H.nb;
        for (unsigned k = 0; k < H.na + H.nb; k++, at++)
            MSCHK(msextargs::resolve_term(R, e, ht[at], nchallenges, n, VB, k < H.na ? &C.a[k] : &C.b[k - H.na], &term_bytes));
    }
    if (n == 0 || next == 0) return MS_OK;
    const size_t nblocks = (n + msext::ROWS - 1) / msext::ROWS;
    if (nblocks > 0x7FFFFFFFull) return fail(MS_ERR_UNSUPPORTED, "%s: column too long", me);
    MSCHK(msextargs::output_overlaps(R, n, VB, VE, d_challenges, nchallenges, d_out, next));
    MSCHK(canon_cols(ctx, me, "d_base", base_field, n, d_base, nbase));
    MSCHK(canon_col(ctx, me, "d_challenges", ext_field, nchallenges, d_challenges));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LockedPoolGuard pooled(ctx);
    void *d_cols = nullptr, *tmp = nullptr;
    MSCHK(pooled.alloc(cols.size() * sizeof(msext::Column), &d_cols));
    MSCHK(pooled.alloc((size_t)next * nblocks * 3 * VE * 8, &tmp));
    MSCHK(stage_upload(ctx, d_cols, cols.data(), cols.size() * sizeof(msext::Column)));
    msext::Params P;
    memset(&P, 0, sizeof P);
    P.cols = (const msext::Column*)d_cols; P.chal = (const uint64_t*)d_challenges;
    P.agg = (uint64_t*)tmp; P.block_state = (uint64_t*)tmp + (size_t)next * nblocks * 2 * VE;
    P.n = n; P.nblocks = (unsigned)nblocks;
    using msstage::FpT; using msstage::Fq3T; using msstage::Fp252T;
    if (VE == 3) ext_launch<Fq3T, FpT>(ctx, P, next, term_bytes);
    else if (VE == 1) ext_launch<FpT, FpT>(ctx, P, next, term_bytes);
    else ext_launch<Fp252T, Fp252T>(ctx, P, next, term_bytes);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
