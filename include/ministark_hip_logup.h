/* ministark_hip_logup.h -- logarithmic-derivative lookup (LogUp) columns, on top of ministark_hip_ext.h (same conventions, same library,
 * the same term layout, init kinds and activity masks): the running sums of fractions
 *     S' = S + m(i) / (alpha - t(i)) - 1 / (alpha - a(i))
 * a lookup argument adds to an AIR between the two trace commitments.  The increment is a QUOTIENT of two linear maps, which
 * ms_build_extension_columns (state' = A(i) state + B(i)) cannot express.  Bindings: rust/gpu/src/hip/sys_logup.rs,
 * ministark_amd/_lib.py `logup_sigs`.
 *
 * ms_build_logup_columns builds `next` columns of n rows of `ext_field` in one asynchronous call (three launches, however many columns;
 * no host wait).  For column e, in exact field arithmetic and equal to this loop bit for bit:
 *     state = init_e
 *     for i in 0..n:  out_e[i] = state                      (inclusive != 0: the state AFTER row i)
 *                     if active_e(i): state = state + sum_{f < nf_e} N_f(i) * inv(D_f(i))
 *     N_f(i) = sum_t sign_t * coef_t * base[col_t][(i + off_t) mod n]     (nn = 0: N = 1)        D_f(i) likewise, nd >= 1
 *     inv(0) = 0     (the library's convention everywhere: gl::mont_inv, the InverseInto stage)
 * d_base, d_challenges, d_out and the terms are those of ms_build_extension_columns.
 * h_columns     next records ms_logup_column (init, init_chal, mask, mask_col, inclusive as in ms_ext_column; nf: the number of fractions)
 * h_fractions   column 0's nf records ms_logup_fraction, then column 1's, ...
 * h_terms       fraction by fraction, in the order of h_fractions: the nn terms (ms_ext_term) of the numerator, then the nd of the denominator
 *   nf = 0      the column holds its init everywhere.
 * Field pairs (base_field -> ext_field): Goldilocks Fp -> Fq3, Fp -> Fp, Fp252 -> Fp252; any other pair is MS_ERR_INVALID.
 * More than MS_LOGUP_MAX_FRACTIONS fractions in a column, more than MS_EXT_MAX_TERMS terms in a numerator or a denominator, or more than
 * MS_LOGUP_MAX_COLUMNS columns: MS_ERR_UNSUPPORTED.
 * n = 0 or next = 0: MS_OK, nothing is touched.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, an unknown field pair, a column / mask /
 * challenge index out of range, an unknown init or mask kind, a sign other than +-1, nd = 0, an output that overlaps a base column, another
 * output or the challenge vector (ms_last_error() contains "overlap").
 * Checked mode (ms_ctx_set_checked): d_base and d_challenges are scanned for non-canonical elements first.
 * While the call runs an output column holds the increments of its rows: it is scratch of the call until the call has completed. */
#ifndef MINISTARK_HIP_LOGUP_H
#define MINISTARK_HIP_LOGUP_H
#include "ministark_hip_ext.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_LOGUP_MAX_FRACTIONS = 4, MS_LOGUP_MAX_COLUMNS = 32 };
typedef struct ms_logup_column { int32_t init; int32_t init_chal; int32_t mask; int32_t mask_col; int32_t inclusive; uint32_t nf; uint32_t pad0; uint32_t pad1; } ms_logup_column;
typedef struct ms_logup_fraction { uint32_t nn; uint32_t nd; } ms_logup_fraction;
int ms_build_logup_columns(ms_ctx* ctx, int base_field, int ext_field, size_t n, const void* const* d_base, unsigned nbase,
                           const void* d_challenges, unsigned nchallenges, const void* h_columns, const void* h_fractions,
                           const void* h_terms, unsigned next, void* const* d_out);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_LOGUP_H */
