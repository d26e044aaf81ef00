// LogUp lookup columns between the two trace commitments -- running sums of fractions: include/ministark_hip_logup.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_logup.h"
#include "logup_kernels.h"

static_assert(mslogup::MAXFRAC == (int)MS_LOGUP_MAX_FRACTIONS && mslogup::MAXCOLS == (int)MS_LOGUP_MAX_COLUMNS && mslogup::MAXTERMS == (int)MS_EXT_MAX_TERMS,
              "logup_kernels.h and the header disagree");
static_assert((int)msext::INIT_CHALLENGE == (int)MS_EXT_INIT_CHALLENGE && (int)msext::MASK_IF_ZERO == (int)MS_EXT_IF_ZERO, "ext_kernels.h and the header disagree");

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
    for (unsigned c = 0; c < nbase; c++) if (!d_base[c]) return fail(MS_ERR_INVALID, "%s: null base column %u", me, c);
    std::vector<mslogup::Column> cols(next);
    size_t fat = 0, at = 0;
    double term_bytes = 0;
    for (unsigned e = 0; e < next; e++) {
        const ms_logup_column& H = hc[e];
        mslogup::Column& C = cols[e];
        memset(&C, 0, sizeof C);
        if (!d_out[e]) return fail(MS_ERR_INVALID, "%s: null output column %u", me, e);
        if (H.init < MS_EXT_INIT_ZERO || H.init > MS_EXT_INIT_CHALLENGE) return fail(MS_ERR_INVALID, "%s: column %u: unknown init kind %d", me, e, H.init);
        if (H.init == MS_EXT_INIT_CHALLENGE && (H.init_chal < 0 || (unsigned)H.init_chal >= nchallenges))
            return fail(MS_ERR_INVALID, "%s: column %u: init challenge %d out of range (%u)", me, e, H.init_chal, nchallenges);
        if (H.mask < MS_EXT_ALWAYS || H.mask > MS_EXT_IF_ZERO) return fail(MS_ERR_INVALID, "%s: column %u: unknown mask kind %d", me, e, H.mask);
        if (H.mask != MS_EXT_ALWAYS && (H.mask_col < 0 || (unsigned)H.mask_col >= nbase))
            return fail(MS_ERR_INVALID, "%s: column %u: mask column %d out of range (%u)", me, e, H.mask_col, nbase);
        C.out = (uint64_t*)d_out[e];
        C.mask = H.mask != MS_EXT_ALWAYS ? (const uint64_t*)d_base[H.mask_col] : nullptr;
        C.nf = H.nf;
        C.mask_kind = H.mask; C.init_kind = H.init; C.init_chal = H.init_chal; C.inclusive = H.inclusive != 0;
        if (H.mask != MS_EXT_ALWAYS) term_bytes += 8.0 * n * VB;
        for (unsigned f = 0; f < H.nf; f++, fat++) {
            const ms_logup_fraction& Q = hf[fat];
            mslogup::Fraction& D = C.f[f];
            if (Q.nd == 0) return fail(MS_ERR_INVALID, "%s: column %u: fraction %u has no denominator term (nd = 0)", me, e, f);
            D.nn = Q.nn; D.nd = Q.nd;
            for (unsigned k = 0; k < Q.nn + Q.nd; k++, at++) {
                const ms_ext_term& T = ht[at];
                msext::Term& R = k < Q.nn ? D.num[k] : D.den[k - Q.nn];
                if (T.col != MS_EXT_NONE && (T.col < 0 || (unsigned)T.col >= nbase)) return fail(MS_ERR_INVALID, "%s: column %u: term column %d out of range (%u)", me, e, T.col, nbase);
                if (T.chal != MS_EXT_NONE && (T.chal < 0 || (unsigned)T.chal >= nchallenges)) return fail(MS_ERR_INVALID, "%s: column %u: term challenge %d out of range (%u)", me, e, T.chal, nchallenges);
                if (T.sign != 1 && T.sign != -1) return fail(MS_ERR_INVALID, "%s: column %u: a term's sign is +1 or -1, not %d", me, e, T.sign);
                R.col = T.col != MS_EXT_NONE ? (const uint64_t*)d_base[T.col] : nullptr;
                if (n) { long long m = (long long)T.off % (long long)n; if (m < 0) m += (long long)n; R.off = (uint64_t)m; }
                R.chal = T.chal; R.sign = T.sign;
                if (R.col) term_bytes += 8.0 * n * VB;
            }
        }
    }
    if (n == 0 || next == 0) return MS_OK;
    const size_t nblocks = (n + mslogup::ROWS - 1) / mslogup::ROWS;
    if (nblocks > 0x7FFFFFFFull) return fail(MS_ERR_UNSUPPORTED, "%s: column too long", me);
    const size_t out_bytes = n * VE * 8;
    for (unsigned e = 0; e < next; e++) {
        for (unsigned c = 0; c < nbase; c++)
            if (ranges_overlap(d_out[e], out_bytes, d_base[c], n * VB * 8)) return fail(MS_ERR_INVALID, "%s: output column %u and base column %u overlap", me, e, c);
        for (unsigned f = 0; f < e; f++)
            if (ranges_overlap(d_out[e], out_bytes, d_out[f], out_bytes)) return fail(MS_ERR_INVALID, "%s: output columns %u and %u overlap", me, f, e);
        if (ranges_overlap(d_out[e], out_bytes, d_challenges, (size_t)nchallenges * VE * 8)) return fail(MS_ERR_INVALID, "%s: output column %u and d_challenges overlap", me, e);
    }
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
