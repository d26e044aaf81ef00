/* ministark_hip_ext.h -- the step between the two trace commitments, on top of ministark_hip.h (same conventions, same library):
 * Trace::build_extension_columns(&challenges) (src/trace.rs; examples/brainfuck/trace.rs:108-289), the running products and running
 * evaluations an AIR builds from its base trace and the challenges drawn after the base commitment.  Like the transcript layer it stands
 * in for an item of the main crate, which is why it has a header -- and generated bindings, rust/gpu/src/hip/sys_ext.rs,
 * ministark_amd/_lib.py `ext_sigs` -- of its own.
 *
 * ms_build_extension_columns builds `next` columns of n rows of `ext_field` in one asynchronous call (three launches, however many
 * columns; no host wait).  For column e, in exact field arithmetic and equal to this loop bit for bit:
 *     state = init_e
 *     for i in 0..n:  out_e[i] = state                      (inclusive != 0: the state AFTER row i)
 *                     if active_e(i): state = A_e(i) * state + B_e(i)
 *     A_e(i) = sum_t sign_t * coef_t * base[col_t][(i + off_t) mod n],     B_e(i) likewise
 * d_base        table of nbase columns of n elements of base_field (Montgomery form).  Only pointers: it need not be the committed trace
 *               (a caller's own indicator column can be appended for a richer mask).
 * d_challenges  nchallenges elements of ext_field in device memory (Montgomery form), read when the kernels run -- e.g. where
 *               ms_coin_draw has just put them.
 * h_columns     next records ms_ext_column, h_terms their terms: column 0's na terms of A, its nb terms of B, column 1's, ...
 *   term        col: index into d_base, or MS_EXT_NONE for a constant term;  off: any int32, wraps mod n;  chal: index into
 *               d_challenges, or MS_EXT_NONE for the literal 1;  sign: +1 or -1.
 *   na = 0      A = 1;   nb = 0: B = 0  (ms_scan_affine's NULL cases).  At most MS_EXT_MAX_TERMS terms per map.
 *   init        MS_EXT_INIT_ZERO, MS_EXT_INIT_ONE, or MS_EXT_INIT_CHALLENGE (the state starts as d_challenges[init_chal])
 *   mask        MS_EXT_ALWAYS; MS_EXT_IF_NONZERO: active where base[mask_col][i] != 0; MS_EXT_IF_ZERO: where it == 0 (the words are
 *               compared: zero is the all-zero element).  An inactive row leaves the state as it is.
 * d_out         next pointers, n elements of ext_field each.
 * Field pairs (base_field -> ext_field): Goldilocks Fp -> Fq3, Fp -> Fp, Fp252 -> Fp252; any other pair is MS_ERR_INVALID.
 * More than MS_EXT_MAX_TERMS terms in a map or more than MS_EXT_MAX_COLUMNS columns: MS_ERR_UNSUPPORTED.
 * n = 0 or next = 0: MS_OK, nothing is touched.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: null tables or a null column, an unknown field pair, a column /
 * mask / challenge index out of range, an unknown init or mask kind, a sign other than +-1, an output that overlaps a base column, another
 * output or the challenge vector (ms_last_error() contains "overlap").
 * Checked mode (ms_ctx_set_checked): d_base and d_challenges are scanned for non-canonical elements first, as by every other arithmetic
 * entry point. */
#ifndef MINISTARK_HIP_EXT_H
#define MINISTARK_HIP_EXT_H
#include "ministark_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_EXT_MAX_TERMS = 8, MS_EXT_MAX_COLUMNS = 32 };
enum { MS_EXT_NONE = -1 };
enum { MS_EXT_INIT_ZERO = 0, MS_EXT_INIT_ONE = 1, MS_EXT_INIT_CHALLENGE = 2 };
enum { MS_EXT_ALWAYS = 0, MS_EXT_IF_NONZERO = 1, MS_EXT_IF_ZERO = 2 };
typedef struct ms_ext_term { int32_t col; int32_t off; int32_t chal; int32_t sign; } ms_ext_term;
typedef struct ms_ext_column { int32_t init; int32_t init_chal; int32_t mask; int32_t mask_col; int32_t inclusive; uint32_t na; uint32_t nb; uint32_t pad; } ms_ext_column;
int ms_build_extension_columns(ms_ctx* ctx, int base_field, int ext_field, size_t n, const void* const* d_base, unsigned nbase,
                               const void* d_challenges, unsigned nchallenges, const void* h_columns, const void* h_terms, unsigned next,
                               void* const* d_out);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_EXT_H */
