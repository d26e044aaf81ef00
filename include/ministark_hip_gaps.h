/* ministark_hip_gaps.h -- deriving a padded table where the trace lies, on top of ministark_hip_ext.h and ministark_hip_sort.h (same
 * conventions, same library, the same activity masks): select rows, insert a dummy row for every clock cycle missing between two rows of a
 * group, and repeat the last row up to the trace length.  examples/brainfuck/vm.rs derive_memory_rows and pad_*_rows: a memory table is
 * ms_sort_rows -> ms_gap_plan -> ms_gap_fill, a plain stable select is the same two calls with counter = -1, plain padding the same two with
 * no mask and no counter.  The step changes the row count; the device decides it and the host need not know it.  Bindings:
 * rust/gpu/src/hip/sys_gaps.rs, ministark_amd/_lib.py `gap_sigs`.
 *
 * ms_gap_plan: one asynchronous call (no host wait).  In exact integers, bit for bit and the same on every run:
 *     row(j)  = d_perm ? perm[j] : j                          for j < n; a row(j) >= n_src is an INACTIVE position: the device cannot refuse
 *                                                             it and never reads out of bounds
 *     act(j)  = row(j) < n_src and the mask holds on base[mask_col][row(j)]
 *     gap(j)  = 0 if counter < 0, or j = n - 1, or act(j) or act(j + 1) is false, or one of the ngroup group columns differs between
 *               row(j) and row(j + 1) (compared as the words lie: equal canonical elements are equal words); otherwise, with
 *               d = canon(base[counter][row(j + 1)]) - canon(base[counter][row(j)]), an INTEGER difference (not mod p; 256 bits over Fp252):
 *                   d >= 2:  gap = min(d - 1, 2^32), and a clipped gap (d - 1 > 2^32) counts in report.saturated
 *                   d  = 1:  gap = 0
 *                   d <= 0:  gap = 0 and j counts in report.unordered; report.first_unordered is the least such j
 *     cnt(j)  = act(j) ? 1 + gap(j) : 0
 *     start[j] = cnt(0) + .. + cnt(j - 1)                      for j <= n: start[n] = report.rows_out
 *     report.active = #{j: act(j)}   report.gaps = #{j: gap(j) > 0}   report.max_gap = max gap(j)
 *     report.first_unordered = 2^64 - 1 when no position is unordered
 * The cap of 2^32 per gap and n <= 2^30 keep every sum below 2^63: that is why the cap exists.  A table with an unordered or a saturated
 * position is not the reference's (its loop would not end on the first): read the report before trusting the rows.
 * d_base        table of nbase columns of n_src elements of `field` (Montgomery form), only pointers, as in ms_sort_rows.
 * h_spec        ONE record ms_gap_spec: group[0 .. ngroup) and counter index d_base (group[ngroup ..) are not read; counter < 0: no gaps);
 *               mask MS_EXT_ALWAYS, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO on base[mask_col], with the meaning they have in ms_ext_column.
 * d_perm        n x uint32 in device memory, e.g. the d_perm of ms_sort_rows, or NULL for the identity.
 * d_start       (n + 1) x uint64.  d_report: one ms_gap_report in device memory.
 * n = 0: MS_OK, start[0] = 0 and a zero report with first_unordered = 2^64 - 1.
 * Scratch, from the context's pool: 8 bytes per 1024 rows (the sums of the tiles) -- under 0.01 bytes per row; cnt(j) is kept in d_start.
 *
 * ms_gap_fill: one asynchronous call.  It reads rows_out = start[n] on the device.  For j < n_out:
 *     jj = min(j, rows_out - 1);   s = the largest position in [0, n) with start[s] <= jj;   k = j - start[s]
 * so rows past rows_out continue the last emitted row: that is the padding.  Destination column c, by h_columns[c].kind (src indexes d_base):
 *     MS_GAP_COPY      base[src][row(s)]
 *     MS_GAP_ZERO      that value when k = 0, a zero element otherwise
 *     MS_GAP_COUNTER   that value plus k, in the field (it may wrap past p; the result is canonical)
 *     MS_GAP_FLAG      src is not read: the field's zero when k = 0, its one otherwise
 * rows_out = 0 (or n = 0): COPY, ZERO and COUNTER store zero elements, FLAG stores one.  Whatever d_start holds, s is clamped to [0, n), a
 * row(s) >= n_src gives a zero element, and nothing is read or written out of bounds.
 * d_dst         ncols (1 .. MS_GAP_MAX_COLUMNS) columns of n_out elements.  n_out = 0: MS_OK, nothing is enqueued.
 *
 * Both: fields MS_GOLDILOCKS_FP and MS_STARK252_FP; MS_GOLDILOCKS_FQ3 is MS_ERR_UNSUPPORTED, and so are n or n_out > 2^30 and n_src > 2^32.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument or column, ngroup > MS_GAP_MAX_GROUP, a column or
 * mask index out of range, an unknown mask or column kind, ncols 0 or above the maximum; d_start or d_report overlapping a column the spec
 * names, the permutation or each other; a destination overlapping a base column a record names, the permutation, d_start or another
 * destination (ms_last_error() contains "overlap").
 * Checked mode (ms_ctx_set_checked): the columns the spec (the column records) name are scanned for non-canonical elements first; the
 * message names d_base, the column's index in it and the row. */
#ifndef MINISTARK_HIP_GAPS_H
#define MINISTARK_HIP_GAPS_H
#include "ministark_hip_sort.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_GAP_MAX_GROUP = 3, MS_GAP_MAX_COLUMNS = 128, MS_GAP_COPY = 0, MS_GAP_ZERO = 1, MS_GAP_COUNTER = 2, MS_GAP_FLAG = 3 };
typedef struct ms_gap_spec { int32_t group[3]; int32_t ngroup; int32_t counter; int32_t mask; int32_t mask_col; int32_t pad0; } ms_gap_spec;
typedef struct ms_gap_report { uint64_t active; uint64_t rows_out; uint64_t gaps; uint64_t max_gap; uint64_t unordered; uint64_t first_unordered; uint64_t saturated; uint64_t pad0; } ms_gap_report;
typedef struct ms_gap_column { int32_t kind; int32_t src; } ms_gap_column;
int ms_gap_plan(ms_ctx* ctx, int field, size_t n_src, const void* const* d_base, unsigned nbase, const void* h_spec, const void* d_perm,
                size_t n, void* d_start, void* d_report);
int ms_gap_fill(ms_ctx* ctx, int field, size_t n_src, const void* const* d_base, unsigned nbase, const void* d_perm, size_t n,
                const void* d_start, const void* h_columns, void* const* d_dst, unsigned ncols, size_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_GAPS_H */
