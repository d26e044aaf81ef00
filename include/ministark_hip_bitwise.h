/* ministark_hip_bitwise.h -- bitwise-operation columns, on top of ministark_hip_range.h (same conventions, same library, the same activity
 * masks; ms_limb_report and ms_lookup_report are the reports here too): the AND, OR or XOR of two columns' canonical integers as a base
 * column, the table (op, x, y, x op y) over all pairs of `bits`-bit limbs that proves such a column limb by limb, and the multiplicities
 * of that table counted straight from the word columns.  Bindings: rust/gpu/src/hip/sys_bitwise.rs, ministark_amd/_lib.py `bitwise_sigs`.
 * WMAX below is 63 for Fp and 251 for Fp252: 2^WMAX is the widest power of two below the modulus, so the OR or XOR of two operands below
 * it is still a canonical integer.
 *
 * ms_bitwise_columns: one asynchronous call (one streaming launch for all the specs, a report; no host wait).  In exact integers, equal
 * to this loop bit for bit and the same on every run:
 *     for k in 0..nspecs: for i in 0..n:
 *         if not active_k(i):  base[dst_k][i] = 0
 *         else:  va, vb = canonical integers of base[a_k][i], base[b_k][i];   active += 1;   W = 2^width_k
 *                base[dst_k][i] = Montgomery form of ((va mod W) op_k (vb mod W))
 *                if va >= W or vb >= W:  overflow += 1;  (first_overflow_spec, first_overflow_row) = min(itself, (k, i))
 * d_base        table of nbase columns of n elements of `field` (Montgomery form), only pointers.  Column dst of a spec is WRITTEN, all n
 *               elements; the others are only read.
 * h_specs       nspecs records ms_bitwise_spec: op, MS_BIT_AND / MS_BIT_OR / MS_BIT_XOR; a, b, the operand columns (a == b is allowed);
 *               dst, the result column; width, the bits of an operand;
 *   mask        MS_EXT_ALWAYS, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO on base[mask_col], with the meaning they have in ms_ext_column.
 * d_report      one ms_limb_report in device memory.  An operand that does not fit `width` bits does not fail the call and its low bits
 *               still go into the result: the report is the finding.  With overflow = 0, first_overflow_spec and first_overflow_row are 0.
 * Limits: width 1 .. WMAX, nspecs <= MS_BITWISE_MAX_SPECS, n <= 2^32.  n = 0 and nspecs = 0: MS_OK, a zero report is written and nothing else.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, a limit broken, an unknown op, a column or
 * mask index out of range, an unknown mask kind, a dst that is -- or whose memory overlaps -- a source or mask column of any spec, two
 * specs with the same dst, d_report overlapping a named column (ms_last_error() contains "overlap").
 * Checked mode (ms_ctx_set_checked): the source and mask columns are scanned for non-canonical elements first; dst may hold anything.
 *
 * ms_bitwise_table: one asynchronous call (one launch).  The table itself, padded by repeating its last row:
 *     T = nops * 4^bits
 *     for j in 0..n_t:  r = min(j, T - 1);  s = r >> (2 bits);  x = (r >> bits) & (2^bits - 1);  y = r & (2^bits - 1)
 *         top[j], tx[j], ty[j], tz[j] = Montgomery forms of ops[s], x, y, x ops[s] y
 * h_ops         nops op codes, int32_t each, distinct: the slot of an op is its position here.
 * d_top         n_t elements, or NULL (an AIR with one op has no op column); d_tx, d_ty, d_tz: n_t elements each.
 * Limits: bits 1 .. MS_BITWISE_MAX_BITS, nops 1 .. 3, T <= 2^24, n_t >= T.  Refused with MS_ERR_INVALID: a null argument, a limit broken,
 * an unknown or repeated op, two outputs that overlap ("overlap").
 *
 * ms_bitwise_multiplicities: one asynchronous call (a count, a conversion; no host wait).  The count reads the WORD columns -- three
 * columns per row, the limb pairs taken from registers -- not 3 nlimbs limb columns.  In exact integers:
 *     T = nops * 4^bits;  cnt = [0] * T;  missing = 0
 *     for s in 0..nsets:  slot = index of op_s in ops;  W = 2^(nlimbs_s * bits)
 *       for i in 0..n: if active_s(i):
 *         va, vb = canonical integers of base[a_s][i], base[b_s][i];   vc = canonical integer of base[c_s][i] if c_s >= 0 else va op_s vb
 *         if va >= W or vb >= W or vc != (va op_s vb):  missing += 1;  (first_missing_set, first_missing_row) = min(itself, (s, i))
 *         else: for j < nlimbs_s:  cnt[slot * 4^bits + (limb_j(va) << bits) + limb_j(vb)] += 1
 *     m[j] = Montgomery form of cnt[j] for j < T;   m[j] = 0 for T <= j < n_m;   duplicate_table_rows = 0
 * (limb_j(v) = (v >> (j bits)) & (2^bits - 1).)  On input with missing = 0 that is, word for word, what ms_lookup_multiplicities at width 4
 * gives over the nlimbs limb-column tuples (op, a_j, b_j, c_j) against ms_bitwise_table's output with n_t = n_m -- without the limb columns,
 * the hash table and the probe walk.
 * h_sets        nsets records ms_bitwise_set: op; a, b, the operand columns; c, the result column to check, or -1 for none; nlimbs; mask.
 * d_m           n_m elements of `field`, T <= n_m.  It may be a column of d_base that no set and no mask names.
 * d_report      one ms_lookup_report in device memory.
 * Limits: bits, nops, T as for the table; nlimbs 1 .. MS_BITWISE_MAX_LIMBS with nlimbs * bits <= WMAX.  MS_ERR_UNSUPPORTED: more than
 * MS_BITWISE_MAX_SETS sets, the sum over the sets of n * nlimbs >= 2^32 (the counters are 32-bit).  nsets = 0 or n = 0: m is all zero and
 * the report is zero.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, a limit broken, n_m < T, an op of a set that
 * is not in h_ops, a column or mask index out of range, an unknown mask kind, d_m or d_report overlapping a column a set or a mask names,
 * or each other (ms_last_error() contains "overlap").
 * Checked mode: the columns the sets and masks name are scanned first.
 * MS_BITWISE_FORM=plain|lds in the environment picks the counting kernel (scripts/bitwise_probe.py); the result does not depend on it.
 * The LDS form exists for bits <= 8 (one op's 4^bits bins are the histogram of a workgroup); `lds` above that is the global form.
 *
 * Fields, all three calls: MS_GOLDILOCKS_FP and MS_STARK252_FP.  MS_GOLDILOCKS_FQ3 is MS_ERR_UNSUPPORTED: base traces are over Fp. */
#ifndef MINISTARK_HIP_BITWISE_H
#define MINISTARK_HIP_BITWISE_H
#include "ministark_hip_range.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_BIT_AND = 0, MS_BIT_OR = 1, MS_BIT_XOR = 2 };
enum { MS_BITWISE_MAX_SPECS = 64, MS_BITWISE_MAX_SETS = 64, MS_BITWISE_MAX_LIMBS = 256, MS_BITWISE_MAX_BITS = 12, MS_BITWISE_MAX_OPS = 3, MS_BITWISE_MAX_TABLE_LOG = 24 };
typedef struct ms_bitwise_spec { int32_t op; int32_t a; int32_t b; int32_t dst; int32_t width; int32_t mask; int32_t mask_col; int32_t pad; } ms_bitwise_spec;
typedef struct ms_bitwise_set { int32_t op; int32_t a; int32_t b; int32_t c; int32_t nlimbs; int32_t mask; int32_t mask_col; int32_t pad; } ms_bitwise_set;
int ms_bitwise_columns(ms_ctx* ctx, int field, size_t n, void* const* d_base, unsigned nbase,
                       const void* h_specs, unsigned nspecs, void* d_report);
int ms_bitwise_table(ms_ctx* ctx, int field, unsigned bits, const void* h_ops, unsigned nops, size_t n_t,
                     void* d_top, void* d_tx, void* d_ty, void* d_tz);
int ms_bitwise_multiplicities(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned bits,
                              const void* h_ops, unsigned nops, const void* h_sets, unsigned nsets, size_t n_m, void* d_m, void* d_report);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_BITWISE_H */
