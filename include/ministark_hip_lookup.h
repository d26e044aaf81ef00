/* ministark_hip_lookup.h -- the multiplicity column of a LogUp lookup, on top of ministark_hip_ext.h (same conventions, same library, the
 * same activity masks): how often every row of a table is looked up.  ms_build_logup_columns (ministark_hip_logup.h) sums
 *     S' = S + m(i) / (alpha - t(i)) - 1 / (alpha - a(i))
 * and m is a column of the BASE trace, committed before alpha is drawn.  ms_lookup_multiplicities counts it where the trace lies, so a
 * trace that is in device memory stays there.  Bindings: rust/gpu/src/hip/sys_lookup.rs, ministark_amd/_lib.py `lookup_sigs`.
 *
 * One asynchronous call (a hash-table build over the table's rows, a probe per looked-up row, a conversion; no host wait).  In exact
 * integers, equal to this loop bit for bit and the same on every run:
 *     first = {}                                   key (the tuple's words) -> smallest active table row that holds it
 *     for j in 0..n: if table_active(j): if key_table(j) in first: duplicate_table_rows += 1   else: first[key_table(j)] = j
 *     cnt = [0] * n;  missing = 0
 *     for s in 0..nsets: for i in 0..n: if active_s(i):
 *         if key_s(i) in first: cnt[first[key_s(i)]] += 1
 *         else: missing += 1;  (first_missing_set, first_missing_row) = min(itself, (s, i))
 *     m[j] = cnt[j] as an element of `field`, Montgomery form
 * d_base        table of nbase columns of n elements of `field` (Montgomery form), only pointers, as in ms_build_extension_columns.
 * width         the number of components of a tuple, 1 .. MS_LOOKUP_MAX_WIDTH.
 * h_table       ONE record ms_lookup_tuple: cols[0 .. width) index d_base and are the table's columns (cols[width ..) are not read).
 * h_lookups     nsets records of the same width: each is one set of looked-up columns; all sets look into the one table.
 *   mask        MS_EXT_ALWAYS, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO on base[mask_col], with the meaning they have in ms_ext_column.  An
 *               inactive table row is not in the table (m = 0, no duplicate); an inactive lookup row is not counted and cannot be missing.
 * Keys are compared word for word, so the input has to be canonical: one value, one key.  Equal active table rows: the one with the
 * smallest index takes all the credit, the others get m = 0 and are counted in duplicate_table_rows.
 * d_m           n elements of `field`.  It may be a column of d_base that no tuple and no mask names (the normal use: the trace's m column).
 * d_report      one ms_lookup_report in device memory, downloaded when the caller wants it.  A looked-up tuple that the table does not
 *               hold does not fail the call (as inv(0) = 0 does not fail ms_build_logup_columns): the report is the finding.  With
 *               missing = 0, first_missing_set and first_missing_row are 0.
 * Fields: MS_GOLDILOCKS_FP and MS_STARK252_FP.  MS_GOLDILOCKS_FQ3 is MS_ERR_UNSUPPORTED: base traces are over Fp.
 * MS_ERR_UNSUPPORTED as well: more than MS_LOOKUP_MAX_SETS sets, n > 2^30, nsets * n >= 2^32 (the counters are 32-bit).
 * n = 0: MS_OK, a zero report is written and nothing else.  nsets = 0: m is all zero (duplicate_table_rows is still counted).
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, width 0 or above the maximum, a column or mask
 * index out of range, an unknown mask kind, d_m or d_report overlapping a column a tuple or a mask names, or each other (ms_last_error()
 * contains "overlap").
 * Checked mode (ms_ctx_set_checked): the columns the tuples and masks name are scanned for non-canonical elements first; the message
 * names d_base, the column's index in it and the row. */
#ifndef MINISTARK_HIP_LOOKUP_H
#define MINISTARK_HIP_LOOKUP_H
#include "ministark_hip_ext.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_LOOKUP_MAX_WIDTH = 4, MS_LOOKUP_MAX_SETS = 8 };
typedef struct ms_lookup_tuple { int32_t cols[4]; int32_t mask; int32_t mask_col; int32_t pad0; int32_t pad1; } ms_lookup_tuple;
typedef struct ms_lookup_report { uint64_t missing; uint64_t first_missing_row; uint32_t first_missing_set; uint32_t pad; uint64_t duplicate_table_rows; } ms_lookup_report;
int ms_lookup_multiplicities(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned width,
                             const void* h_table, const void* h_lookups, unsigned nsets, void* d_m, void* d_report);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_LOOKUP_H */
