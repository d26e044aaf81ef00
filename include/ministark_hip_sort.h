/* ministark_hip_sort.h -- ordering the rows of a trace where it lies, on top of ministark_hip_ext.h (same conventions, same library, the same
 * activity masks): the permutation that sorts rows by a key of 1 .. 4 base columns, and a gather of columns by an index in device memory.
 * A memory table sorted by (address, cycle), an instruction table sorted by address, the "same rows in another order" columns of a
 * permutation argument: a trace that is in device memory stays there.  Bindings: rust/gpu/src/hip/sys_sort.rs, ministark_amd/_lib.py
 * `sort_sigs`.
 *
 * ms_sort_rows: one asynchronous call (no host wait).  In exact integers, bit for bit and the same on every run:
 *     canon(c, i) = the canonical integer of base[c][i]                       (OUT of Montgomery form)
 *     act  = [i for i in range(n) if active(i)];   ina = [i for i in range(n) if not active(i)]
 *     perm = sorted(act, key = lambda i: tuple(canon(cols[k], i) for k in range(nkeys))) + ina
 *     report.active = len(act)
 *     report.varying_bytes = the number of (key component k, byte b of its little-endian canonical value) at which two active rows differ
 * The sort is stable: active rows of equal keys keep their original order; the inactive rows follow, in their original order.
 * d_base        table of nbase columns of n elements of `field` (Montgomery form), only pointers, as in ms_build_extension_columns.
 * nkeys         the number of components of the key, 1 .. MS_SORT_MAX_KEYS.
 * h_key         ONE record ms_sort_key: cols[0 .. nkeys) index d_base (cols[nkeys ..) are not read); cols[0] is the most significant
 *               component.  Ascending order, as integers in [0, p).
 *   mask        MS_EXT_ALWAYS, MS_EXT_IF_NONZERO, MS_EXT_IF_ZERO on base[mask_col], with the meaning they have in ms_ext_column.
 * d_perm        n x uint32: perm[j] is the row that comes j-th.
 * d_report      one ms_sort_report in device memory, downloaded when the caller wants it.  varying_bytes is also the number of radix-256
 *               passes the call executed: its cost follows the bytes that differ, not the width of the key.
 * Fields: MS_GOLDILOCKS_FP and MS_STARK252_FP.  MS_GOLDILOCKS_FQ3 is MS_ERR_UNSUPPORTED: base traces are over Fp.
 * MS_ERR_UNSUPPORTED as well: n > 2^30 (an index is 32 bits).  n = 0: MS_OK, a zero report is written and nothing else.
 * Refused with MS_ERR_INVALID before anything is enqueued, nothing written: a null argument, nkeys 0 or above the maximum, a column or mask
 * index out of range, an unknown mask kind, d_perm or d_report overlapping a column the key or the mask names, or each other
 * (ms_last_error() contains "overlap").
 * Checked mode (ms_ctx_set_checked): the columns the key and the mask name are scanned for non-canonical elements first; the message names
 * d_base, the column's index in it and the row.  A non-canonical key has no defined order.
 * Scratch, from the context's pool, per row: 8 bytes per word of the key (nkeys words over Fp, 4 nkeys over Fp252) for the canonical key,
 * 16 for the two buffers of the current word, 4 for the second index buffer, 0.5 for the tile histograms, 1 for the mask if there is one;
 * about 2 KiB besides.
 *
 * ms_permute_columns: dst[c][i] = src[c][index[i]] for i < n_out, c < ncols -- one asynchronous launch.  A gather: the index may repeat rows
 * and need not cover them.  An entry >= n_src reads nothing and stores a zero element (the device cannot refuse; it never reads out of
 * bounds).  All three fields; ncols 1 .. MS_PERMUTE_MAX_COLUMNS; n_src <= 2^32.  n_out = 0: MS_OK, nothing is enqueued.
 * d_src, d_dst  tables of ncols pointers: columns of n_src and of n_out elements of `field`.
 * d_index       n_out x uint32 in device memory, e.g. the d_perm of ms_sort_rows.
 * Refused with MS_ERR_INVALID before anything is enqueued: a null argument or column, ncols 0 or above the maximum, a d_dst[c] that
 * overlaps any source column, the index or another destination ("overlap"). */
#ifndef MINISTARK_HIP_SORT_H
#define MINISTARK_HIP_SORT_H
#include "ministark_hip_ext.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { MS_SORT_MAX_KEYS = 4, MS_PERMUTE_MAX_COLUMNS = 128 };
typedef struct ms_sort_key { int32_t cols[4]; int32_t mask; int32_t mask_col; int32_t pad0; int32_t pad1; } ms_sort_key;
typedef struct ms_sort_report { uint64_t active; uint64_t varying_bytes; } ms_sort_report;
int ms_sort_rows(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned nkeys, const void* h_key,
                 void* d_perm, void* d_report);
int ms_permute_columns(ms_ctx* ctx, int field, size_t n_src, const void* const* d_src, void* const* d_dst, unsigned ncols,
                       const void* d_index, size_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* MINISTARK_HIP_SORT_H */
