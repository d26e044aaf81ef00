// The argument checks ms_build_extension_columns (ms_ext.cpp) and ms_build_logup_columns (ms_logup.cpp) share: both take ms_ext_column's
// first five words (init, init_chal, mask, mask_col, inclusive), ms_ext_term records, one output per column and the challenge vector.
// Each function refuses in the order the entry points always have: the first bad word of the first bad column is the one reported.
#pragma once
#include "ms_internal.h"
#include "../../include/ministark_hip_ext.h"
#include "ext_kernels.h"

namespace msextargs {

// the output, init and mask of column e (H: ms_ext_column or ms_logup_column) -> the kernel's record C; the mask column's bytes -> *term_bytes
template <class H, class C>
static int column_header(BaseColumns& R, unsigned e, const H& h, unsigned nchallenges, void* d_out, size_t n, unsigned VB, C* c, double* term_bytes) {
    if (!d_out) return fail(MS_ERR_INVALID, "%s: null output column %u", R.me, e);
    if (h.init < MS_EXT_INIT_ZERO || h.init > MS_EXT_INIT_CHALLENGE) return fail(MS_ERR_INVALID, "%s: column %u: unknown init kind %d", R.me, e, h.init);
    if (h.init == MS_EXT_INIT_CHALLENGE && (h.init_chal < 0 || (unsigned)h.init_chal >= nchallenges))
        return fail(MS_ERR_INVALID, "%s: column %u: init challenge %d out of range (%u)", R.me, e, h.init_chal, nchallenges);
    char who[32];
    snprintf(who, sizeof who, "column %u: ", e);
    MSCHK(R.mask(h.mask, h.mask_col, who, &c->mask));
    c->out = (uint64_t*)d_out;
    c->mask_kind = h.mask; c->init_kind = h.init; c->init_chal = h.init_chal; c->inclusive = h.inclusive != 0;
    if (c->mask) *term_bytes += 8.0 * n * VB;
    return MS_OK;
}

// one term of column e -> D: its column's address, its offset reduced to [0, n), challenge and sign; a column term's bytes -> *term_bytes
static int resolve_term(BaseColumns& R, unsigned e, const ms_ext_term& T, unsigned nchallenges, size_t n, unsigned VB, msext::Term* D, double* term_bytes) {
    char what[32];
    snprintf(what, sizeof what, "column %u: term ", e);
    D->col = nullptr;
    if (T.col != MS_EXT_NONE) MSCHK(R.col(T.col, what, &D->col));
    if (T.chal != MS_EXT_NONE && (T.chal < 0 || (unsigned)T.chal >= nchallenges)) return fail(MS_ERR_INVALID, "%s: column %u: term challenge %d out of range (%u)", R.me, e, T.chal, nchallenges);
    if (T.sign != 1 && T.sign != -1) return fail(MS_ERR_INVALID, "%s: column %u: a term's sign is +1 or -1, not %d", R.me, e, T.sign);
    if (n) { long long m = (long long)T.off % (long long)n; if (m < 0) m += (long long)n; D->off = (uint64_t)m; }
    D->chal = T.chal; D->sign = T.sign;
    if (D->col) *term_bytes += 8.0 * n * VB;
    return MS_OK;
}

// every output against every base column (named by a term or not), the outputs before it and the challenges
static int output_overlaps(const BaseColumns& R, size_t n, unsigned VB, unsigned VE, const void* d_challenges, unsigned nchallenges, void* const* d_out, unsigned next) {
    const size_t out_bytes = n * VE * 8;
    for (unsigned e = 0; e < next; e++) {
        for (unsigned c = 0; c < R.nbase; c++)
            if (ranges_overlap(d_out[e], out_bytes, R.d_base[c], n * VB * 8)) return fail(MS_ERR_INVALID, "%s: output column %u and base column %u overlap", R.me, e, c);
        for (unsigned f = 0; f < e; f++)
            if (ranges_overlap(d_out[e], out_bytes, d_out[f], out_bytes)) return fail(MS_ERR_INVALID, "%s: output columns %u and %u overlap", R.me, f, e);
        if (ranges_overlap(d_out[e], out_bytes, d_challenges, (size_t)nchallenges * VE * 8)) return fail(MS_ERR_INVALID, "%s: output column %u and d_challenges overlap", R.me, e);
    }
    return MS_OK;
}

}  // namespace msextargs
