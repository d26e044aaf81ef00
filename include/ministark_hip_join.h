/* ministark_hip_join.h -- join rows against a table: for every row, WHICH table row holds its key, on top of ministark_hip_ext.h (same
 * conventions, same library, the same activity masks) and of ministark_hip_lookup.h, whose ms_lookup_tuple is the key record here.
 * ms_lookup_multiplicities finds the table row of every looked-up row and only counts it; ms_join_rows writes that row's index, and
 * ms_permute_columns (ministark_hip_sort.h) then fetches the table's other columns by it: instruction fetch by ip from a program table,
 * opcode decode, the result column of a function table, any ROM read.  The table has a side of its own -- a program of L rows is not a
 * trace of n rows.  Bindings: rust/gpu/src/hip/sys_join.rs, ministark_amd/_lib.py `join_sigs`.
 *
 * One asynchronous call (a hash-table build over the table's rows, a probe per joined row, a report; no host wait).  In exact integers,
 * equal to this loop bit for bit and the same on every run:
 *     first = {}; dup = 0; tact = 0                key (the tuple's words) -> smallest active table row that holds it
 *     for j in 0..n_table: if table_active(j): tact += 1; if key_table(j) in first: dup += 1  else: first[key_table(j)] = j
 *     for s in 0..nsets: for i in 0..n:
 *         if not active_s(i):            match[s][i] = MS_JOIN_NONE
 *         elif key_s(i) in first:        match[s][i] = first[key_s(i)];  matched += 1
 *         else:                          match[s][i] = MS_JOIN_NONE;  missing += 1;  (first_missing_set, first_missing_row) = min(itself, (s, i))
 *     duplicate_table_rows = dup;  table_active = tact
 * d_table       table of ntable_cols columns of n_table elements of `field` (Montgomery form), only pointers.
 * d_base        table of nbase columns of n elements of `field`.  It may be d_table itself with n_table == n: a self-join.
 * width         the number of components of a key, 1 .. MS_JOIN_MAX_WIDTH.
 * h_table_key   ONE record ms_lookup_tuple: cols[0 .. width) and the mask index d_table (cols[width ..) are not read).
 * h_keys        nsets records of the same width whose cols and masks index d_base: each is one set of joined columns.
 *   mask        MS_EXT_ALWAYS, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO on the side's own column mask_col, with the meaning they have in
 *               ms_ext_column.  An inactive table row is not in the table; an inactive joined row matches nothing and cannot be missing.
 * Keys are compared word for word on Montgomery words, so the input has to be canonical: one value, one key.  Equal active table rows:
 * the one with the smallest index is the match, the others are counted in duplicate_table_rows.
 * d_match       HOST array of nsets device pointers, each to n uint32: the matched table row, or MS_JOIN_NONE -- an index past any table,
 *               for which ms_permute_columns stores a zero element.  Every one of the n entries of every set is written.
 * d_report      one ms_join_report in device memory, downloaded when the caller wants it.  A key that the table does not hold does not
 *               fail the call: the report is the finding.  With missing = 0, first_missing_set and first_missing_row are 0.
 * Fields: MS_GOLDILOCKS_FP and MS_STARK252_FP.  MS_GOLDILOCKS_FQ3 is MS_ERR_UNSUPPORTED: traces and tables are over Fp.
 * MS_ERR_UNSUPPORTED as well: more than MS_JOIN_MAX_SETS sets, n_table > 2^30 (a slot is a 32-bit row index and MS_JOIN_NONE the
 * sentinel), n > 2^32 (first_missing_row travels packed as set << 32 | row).
 * n_table = 0 and n = 0: MS_OK, following the loop -- an empty table makes every active row missing; n = 0 still counts table_active and
 * duplicate_table_rows.  nsets = 0: MS_OK, only the report is written.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument or a null d_match[s], width 0 or above the
 * maximum, a column or mask index out of range on either side (the message says which side and which set), an unknown mask kind, a
 * d_match[s] or d_report overlapping a column a key or a mask names on either side, another d_match, or the report (ms_last_error()
 * contains "overlap").
 * Checked mode (ms_ctx_set_checked): the columns the keys and masks name, on both sides, are scanned for non-canonical elements first; the
 * message names d_table or d_base, the column's index in it and the row. */
#ifndef MINISTARK_HIP_JOIN_H
#define MINISTARK_HIP_JOIN_H
#include "ministark_hip_ext.h"
#include "ministark_hip_lookup.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_JOIN_MAX_WIDTH = 4, MS_JOIN_MAX_SETS = 8 };
#define MS_JOIN_NONE 0xFFFFFFFFu
typedef struct ms_join_report { uint64_t matched; uint64_t missing; uint64_t first_missing_row; uint32_t first_missing_set; uint32_t pad; uint64_t duplicate_table_rows; uint64_t table_active; } ms_join_report;
int ms_join_rows(ms_ctx* ctx, int field, size_t n_table, const void* const* d_table, unsigned ntable_cols, const void* h_table_key,
                 size_t n, const void* const* d_base, unsigned nbase, unsigned width,
                 const void* h_keys, unsigned nsets, void* const* d_match, void* d_report);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_JOIN_H */
