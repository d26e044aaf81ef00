// LogUp lookup columns between the two trace commitments -- running sums of fractions: include/ministark_hip_logup.h.
#include "ext_args.h"
#include "../../include/ministark_hip_logup.h"
#include "logup_kernels.h"

static_assert(mslogup::MAXFRAC == (int)MS_LOGUP_MAX_FRACTIONS && mslogup::MAXCOLS == (int)MS_LOGUP_MAX_COLUMNS && mslogup::MAXTERMS == (int)MS_EXT_MAX_TERMS,
              "logup_kernels.h and the header disagree");

template <class F, class B>
static void logup_launch(ms_ctx* ctx, const mslogup::Params& P, unsigned next, double term_bytes) {
    using namespace mslogup;
    const double col_bytes = 8.0 * P.n * F::V * next;
    { ProfScope ps(ctx, "logup_increments", term_bytes + col_bytes);
      hipLaunchKernelGGL((logup_increments<F, B>), dim3(P.nblocks, next), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "logup_blocks", 0.0);
      hipLaunchKernelGGL((logup_blocks<F>), dim3(next), dim3(NT), 0, ctx->stream, P); }
    { ProfScope ps(ctx, "logup_apply", 2.0 * col_bytes);
      hipLaunchKernelGGL((logup_apply<F>), dim3(P.nblocks, next), dim3(NT), 0, ctx->stream, P); }
}

extern "C" int ms_build_logup_columns(ms_ctx* ctx, int base_field, int ext_field, size_t n, const void* const* d_base, unsigned nbase,
                                      const void* d_challenges, unsigned nchallenges, const void* h_columns, const void* h_fractions,
                                      const void* h_terms, unsigned next, void* const* d_out) {
    const char* me = "ms_build_logup_columns";
    if (!ctx || (nbase && !d_base) || (nchallenges && !d_challenges) || (next && (!h_columns || !d_out))) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned VB = 0, VE = 0;
    if (field_words(base_field, &VB) != MS_OK || field_words(ext_field, &VE) != MS_OK || VB == 3 || (VB == 4) != (VE == 4))
        return fail(MS_ERR_INVALID, "%s: the field pair (base %d, extension %d) is not one of Fp -> Fq3, Fp -> Fp, Fp252 -> Fp252", me, base_field, ext_field);
    if (next > (unsigned)MS_LOGUP_MAX_COLUMNS) return fail(MS_ERR_UNSUPPORTED, "%s: %u columns in one call (at most %d)", me, next, MS_LOGUP_MAX_COLUMNS);
    const ms_logup_column* hc = (const ms_logup_column*)h_columns;
    const ms_logup_fraction* hf = (const ms_logup_fraction*)h_fractions;
    const ms_ext_term* ht = (const ms_ext_term*)h_terms;
    size_t nfrac = 0;
    for (unsigned e = 0; e < next; e++) {
        if (hc[e].nf > (unsigned)MS_LOGUP_MAX_FRACTIONS)
            return fail(MS_ERR_UNSUPPORTED, "%s: column %u has %u fractions (at most %d)", me, e, hc[e].nf, MS_LOGUP_MAX_FRACTIONS);
        nfrac += hc[e].nf;
    }
    if (nfrac && (!hf || !ht)) return fail(MS_ERR_INVALID, "%s: null argument", me);
    for (size_t k = 0; k < nfrac; k++)
        if (hf[k].nn > (unsigned)MS_EXT_MAX_TERMS || hf[k].nd > (unsigned)MS_EXT_MAX_TERMS)
            return fail(MS_ERR_UNSUPPORTED, "%s: fraction %zu has %u / %u terms (at most %d in a numerator or a denominator)", me, k, hf[k].nn, hf[k].nd, MS_EXT_MAX_TERMS);
    BaseColumns R(me, d_base, nbase);
    MSCHK(R.null_check());
    std::vector<mslogup::Column> cols(next);
    size_t fat = 0, at = 0;
    double term_bytes = 0;
    for (unsigned e = 0; e < next; e++) {
        const ms_logup_column& H = hc[e];
        mslogup::Column& C = cols[e];
        memset(&C, 0, sizeof C);
        MSCHK(msextargs::column_header(R, e, H, nchallenges, d_out[e], n, VB, &C, &term_bytes));
        C.nf = H.nf;
        for (unsigned f = 0; f < H.nf; f++, fat++) {
            const ms_logup_fraction& Q = hf[fat];
            mslogup::Fraction& D = C.f[f];
            if (Q.nd == 0) return fail(MS_ERR_INVALID, "%s: column %u: fraction %u has no denominator term (nd = 0)", me, e, f);
            D.nn = Q.nn; D.nd = Q.nd;
            for (unsigned k = 0; k < Q.nn + Q.nd; k++, at++)
                MSCHK(msextargs::resolve_term(R, e, ht[at], nchallenges, n, VB, k < Q.nn ? &D.num[k] : &D.den[k - Q.nn], &term_bytes));
        }
    }
    if (n == 0 || next == 0) return MS_OK;
    const size_t nblocks = (n + mslogup::ROWS - 1) / mslogup::ROWS;
    if (nblocks > 0x7FFFFFFFull) return fail(MS_ERR_UNSUPPORTED, "%s: column too long", me);
    MSCHK(msextargs::output_overlaps(R, n, VB, VE, d_challenges, nchallenges, d_out, next));
    MSCHK(canon_cols(ctx, me, "d_base", base_field, n, d_base, nbase));
    MSCHK(canon_col(ctx, me, "d_challenges", ext_field, nchallenges, d_challenges));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LockedPoolGuard pooled(ctx);
    void *d_cols = nullptr, *tmp = nullptr;
    MSCHK(pooled.alloc(cols.size() * sizeof(mslogup::Column), &d_cols));
    MSCHK(pooled.alloc((size_t)next * nblocks * 2 * VE * 8, &tmp));
    MSCHK(stage_upload(ctx, d_cols, cols.data(), cols.size() * sizeof(mslogup::Column)));
    mslogup::Params P;
    memset(&P, 0, sizeof P);
    P.cols = (const mslogup::Column*)d_cols; P.chal = (const uint64_t*)d_challenges;
    P.agg = (uint64_t*)tmp; P.block_state = (uint64_t*)tmp + (size_t)next * nblocks * VE;
    P.n = n; P.nblocks = (unsigned)nblocks;
    using msstage::FpT; using msstage::Fq3T; using msstage::Fp252T;
    if (VE == 3) logup_launch<Fq3T, FpT>(ctx, P, next, term_bytes);
    else if (VE == 1) logup_launch<FpT, FpT>(ctx, P, next, term_bytes);
    else logup_launch<Fp252T, Fp252T>(ctx, P, next, term_bytes);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
