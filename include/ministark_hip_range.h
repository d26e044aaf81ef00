/* ministark_hip_range.h -- range-check columns, on top of ministark_hip_ext.h (same conventions, same library, the same activity masks)
 * and of ministark_hip_lookup.h, whose ms_lookup_report is the report of the count here: the limbs of a value column as base columns,
 * and the multiplicities of the table 0 .. 2^bits - 1 those limbs are looked up in.  "This 32-bit value is two 16-bit limbs and every limb
 * is in [0, 2^16)" is then two calls on a trace that stays in device memory.  Bindings: rust/gpu/src/hip/sys_range.rs,
 * ministark_amd/_lib.py `range_sigs`.
 *
 * ms_limb_decompose: one asynchronous call (one streaming launch for all the specs, a report; no host wait).  In exact integers, equal
 * to this loop bit for bit and the same on every run:
 *     for k in 0..nspecs: for i in 0..n:
 *         if not active_k(i):  base[dst0_k + j][i] = 0 for every j < nlimbs_k
 *         else:  v = canonical integer of base[src_k][i];   active += 1
 *                base[dst0_k + j][i] = Montgomery form of ((v >> (j * bits_k)) & (2^bits_k - 1)),  j < nlimbs_k
 *                if v >> (nlimbs_k * bits_k) != 0:  overflow += 1;  (first_overflow_spec, first_overflow_row) = min(itself, (k, i))
 * d_base        table of nbase columns of n elements of `field` (Montgomery form), only pointers.  The columns dst0 .. dst0 + nlimbs - 1
 *               of a spec are WRITTEN, all n elements of each; the others are only read.
 * h_specs       nspecs records ms_limb_spec: src, the value column; dst0, nlimbs, the destination columns; bits, the width of a limb;
 *   mask        MS_EXT_ALWAYS, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO on base[mask_col], with the meaning they have in ms_ext_column.
 * d_report      one ms_limb_report in device memory, downloaded when the caller wants it.  A value that does not fit its limbs does not
 *               fail the call and still gets its low limbs: the report is the finding, as `missing` is for lookups.  With overflow = 0,
 *               first_overflow_spec and first_overflow_row are 0.
 * Limits: bits 1 .. MS_RANGE_MAX_LIMB_BITS, nlimbs 1 .. MS_RANGE_MAX_LIMBS, nlimbs * bits <= 64 V (V = 1 for Fp, 4 for Fp252),
 * nspecs <= MS_RANGE_MAX_SPECS, n <= 2^32.  n = 0 and nspecs = 0: MS_OK, a zero report is written and nothing else.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, a limit broken, a column or mask index out
 * of range (dst0 + nlimbs past the table included), an unknown mask kind, a destination column that is -- or whose memory overlaps -- a
 * source or mask column of any spec, destination ranges of two specs that intersect, d_report overlapping a named column
 * (ms_last_error() contains "overlap").
 * Checked mode (ms_ctx_set_checked): the source and mask columns are scanned for non-canonical elements first; the destinations may
 * hold anything.
 *
 * ms_range_multiplicities: one asynchronous call (a count, a conversion; no host wait).  In exact integers:
 *     cnt = [0] * 2^bits;  missing = 0
 *     for s in 0..nsets: for i in 0..n: if active_s(i):
 *         v = canonical integer of base[col_s][i]
 *         if v < 2^bits: cnt[v] += 1   else: missing += 1;  (first_missing_set, first_missing_row) = min(itself, (s, i))
 *     m[j] = Montgomery form of cnt[j] for j < 2^bits;   m[j] = 0 for 2^bits <= j < n_m;   duplicate_table_rows = 0
 * With n_m = n that is, word for word, what ms_lookup_multiplicities at width 1 gives against the table column t[j] = min(j, 2^bits - 1)
 * -- without the table column, the hash table built over it and the probe walk.
 * h_sets        nsets records ms_range_set: col, the looked-up column; mask, mask_col as above.
 * d_m           n_m elements of `field`, 2^bits <= n_m.  It may be a column of d_base that no set and no mask names.
 * d_report      one ms_lookup_report in device memory.
 * Limits: bits 1 .. MS_RANGE_MAX_TABLE_BITS.  MS_ERR_UNSUPPORTED: more than MS_RANGE_MAX_SETS sets, nsets * n >= 2^32 (the counters are
 * 32-bit).  nsets = 0 or n = 0: m is all zero and the report is zero.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, bits out of range, n_m < 2^bits, a column or
 * mask index out of range, an unknown mask kind, d_m or d_report overlapping a column a set or a mask names, or each other
 * (ms_last_error() contains "overlap").
 * Checked mode: the columns the sets and masks name are scanned first; the message names d_base, the column's index in it and the row.
 * MS_RANGE_FORM=plain|lds in the environment picks the counting kernel (scripts/range_probe.py); the result does not depend on it.
 *
 * Fields, both calls: MS_GOLDILOCKS_FP and MS_STARK252_FP.  MS_GOLDILOCKS_FQ3 is MS_ERR_UNSUPPORTED: base traces are over Fp. */
#ifndef MINISTARK_HIP_RANGE_H
#define MINISTARK_HIP_RANGE_H
#include "ministark_hip_ext.h"
#include "ministark_hip_lookup.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_RANGE_MAX_SPECS = 64, MS_RANGE_MAX_SETS = 64, MS_RANGE_MAX_LIMBS = 256, MS_RANGE_MAX_LIMB_BITS = 32, MS_RANGE_MAX_TABLE_BITS = 24 };
typedef struct ms_limb_spec { int32_t src; int32_t dst0; int32_t nlimbs; int32_t bits; int32_t mask; int32_t mask_col; int32_t pad0; int32_t pad1; } ms_limb_spec;
typedef struct ms_range_set { int32_t col; int32_t mask; int32_t mask_col; int32_t pad; } ms_range_set;
typedef struct ms_limb_report { uint64_t overflow; uint64_t first_overflow_row; uint32_t first_overflow_spec; uint32_t pad; uint64_t active; } ms_limb_report;
int ms_limb_decompose(ms_ctx* ctx, int field, size_t n, void* const* d_base, unsigned nbase,
                      const void* h_specs, unsigned nspecs, void* d_report);
int ms_range_multiplicities(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned bits,
                            const void* h_sets, unsigned nsets, size_t n_m, void* d_m, void* d_report);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_RANGE_H */
