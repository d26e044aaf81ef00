"""`Trace::build_extension_columns(&challenges)` (src/trace.rs; examples/brainfuck/trace.rs:108-289) over ms_build_extension_columns
(include/ministark_hip_ext.h): every extension column of an AIR -- running products, running evaluations -- in ONE asynchronous call, the
challenges read where the device-resident coin drew them.

    state = init;  for row i: out[i] = state;  if active(i): state = A(i) * state + B(i)
    A(i) = sum_t sign_t * coef_t * base[col_t][(i + off_t) mod n],   B(i) likewise

A term is a tuple (sign, challenge, column, offset): sign +1 / -1; challenge an index into the challenge vector or None for the literal 1;
column an index into the base matrix or None for a constant term; offset any integer (wraps mod n; may be left out: 0).

Logarithmic-derivative lookups (LogUp) are running sums of FRACTIONS of such linear maps, which the affine rule cannot express:
`LogUpColumn` over ms_build_logup_columns (include/ministark_hip_logup.h), with the same terms, inits and masks:

    state = init;  for row i: out[i] = state;  if active(i): state = state + sum_f N_f(i) * inv(D_f(i)),   inv(0) = 0

`build_extension_columns` takes a list that mixes both kinds: one call of each, the columns returned in the order listed.

The m of a lookup -- how often each table row is looked up -- is a column of the BASE trace: `lookup_multiplicities` over
ms_lookup_multiplicities (include/ministark_hip_lookup.h) counts it on the device, and its `LookupReport` names a looked-up tuple that the
table does not hold.

Ordering rows -- a memory table by (address, cycle), the permuted columns of a permutation argument -- is `sort_rows` over ms_sort_rows and
`permute_columns` over ms_permute_columns (include/ministark_hip_sort.h): the permutation is computed and applied in device memory.

A table whose row count differs from its source's -- the rows a mask selects, a dummy row for every clock cycle missing between two rows of
an address, padding up to the trace length -- is `gap_plan` over ms_gap_plan and `gap_fill` over ms_gap_fill
(include/ministark_hip_gaps.h): the device decides the row count and writes the rows.

Fetching -- the instruction at an ip, the value at a ROM address, the result column of a function table -- is `join_rows` over ms_join_rows
(include/ministark_hip_join.h): for every row, the index of the table row that holds its key, the table a matrix of its own; and
`fetch_columns`, which hands that index to `permute_columns` and returns the table's other columns row by row.

Range checks -- "this 32-bit value is two 16-bit limbs, and every limb is in [0, 2^16)" -- are `limb_decompose` over ms_limb_decompose and
`range_multiplicities` over ms_range_multiplicities (include/ministark_hip_range.h): the limb columns written where the value column lies,
and the multiplicities of the table 0 .. 2^bits - 1 counted by direct indexing, with no table column and no hash table.

Bitwise operations -- the one family of columns no constraint program can compute -- are `bitwise_columns` over ms_bitwise_columns,
`bitwise_table` over ms_bitwise_table and `bitwise_multiplicities` over ms_bitwise_multiplicities (include/ministark_hip_bitwise.h):
c = a AND / OR / XOR b on the canonical integers of two columns, the table (op, x, y, x op y) over all pairs of `bits`-bit limbs written on
the device, and that table's multiplicities counted straight from the word columns a, b, c -- the limb pairs are taken from registers."""
import ctypes

import numpy as np

from ._lib import (BitwiseSetRecord, BitwiseSpecRecord, GapColumnRecord, GapReportRecord, GapSpecRecord, JoinReportRecord, LimbReportRecord, LimbSpecRecord, LookupReportRecord, LookupTupleRecord,
                   RangeSetRecord, SortKeyRecord, SortReportRecord)
from .api import FIELD_WORDS, GOLDILOCKS_FP, STARK252_FP, DeviceBytes, GpuVec, Matrix, _ptr_array, f252_from_mont_limbs, gl_from_mont

MAX_TERMS, MAX_COLUMNS, NONE = 8, 32, -1
ROWS_PER_WORKGROUP = 1024             # msext::ROWS (csrc/ext_kernels.h): the rows one workgroup scans; tests/test_ext_abi.py keeps the two equal
_INIT = {0: 0, 1: 1}
_MASK = {"nonzero": 1, "zero": 2}
LOGUP_MAX_FRACTIONS, LOGUP_MAX_COLUMNS = 4, 32
LOOKUP_MAX_WIDTH, LOOKUP_MAX_SETS = 4, 8
SORT_MAX_KEYS, PERMUTE_MAX_COLUMNS = 4, 128
JOIN_MAX_WIDTH, JOIN_MAX_SETS, JOIN_NONE = 4, 8, 0xFFFFFFFF
RANGE_MAX_SPECS, RANGE_MAX_SETS, RANGE_MAX_LIMBS, RANGE_MAX_LIMB_BITS, RANGE_MAX_TABLE_BITS = 64, 64, 256, 32, 24
BITWISE_MAX_SPECS, BITWISE_MAX_SETS, BITWISE_MAX_LIMBS, BITWISE_MAX_BITS, BITWISE_MAX_OPS, BITWISE_MAX_TABLE_LOG = 64, 64, 256, 12, 3, 24
BITWISE_OPS = {"and": 0, "or": 1, "xor": 2}                      # MS_BIT_AND, MS_BIT_OR, MS_BIT_XOR
BITWISE_WMAX = {GOLDILOCKS_FP: 63, STARK252_FP: 251}             # 2^WMAX is the widest power of two below the modulus


def _mask_words(who, mask):
    """mask=None | ("nonzero", m) | ("zero", m) of class `who` -> (kind, column): the mask and mask_col words of its record"""
    if mask is None:
        return (0, 0)
    if len(mask) != 2 or mask[0] not in _MASK:
        raise ValueError(f"{who}: mask is None, ('nonzero', m) or ('zero', m), not {mask!r}")
    return (_MASK[mask[0]], int(mask[1]))


class ExtColumn:
    """One extension column.  init: 0, 1, or ("challenge", k);  a_terms / b_terms: lists of terms (an empty A is 1, an empty B is 0);
    mask: None (every row is active), ("nonzero", m) or ("zero", m): active where base column m is != 0 / == 0 (the processor and memory
    tables' padding rules, trace.rs:135, 184);  inclusive: out[i] is the state AFTER row i."""

    def __init__(self, init, a_terms, b_terms, mask=None, inclusive=False):
        self.init, self.a_terms, self.b_terms, self.mask, self.inclusive = init, list(a_terms), list(b_terms), mask, bool(inclusive)

    def _head(self):
        """[init, init_chal, mask, mask_col, inclusive]: the first five words of ms_ext_column and of ms_logup_column"""
        who = type(self).__name__
        if isinstance(self.init, tuple):
            kind, k = self.init
            if kind != "challenge":
                raise ValueError(f"{who}: init is 0, 1 or ('challenge', k), not {self.init!r}")
            init = (2, int(k))
        elif self.init in _INIT:
            init = (_INIT[self.init], 0)
        else:
            raise ValueError(f"{who}: init is 0, 1 or ('challenge', k), not {self.init!r}")
        mask = _mask_words(who, self.mask)
        return [init[0], init[1], mask[0], mask[1], int(self.inclusive)]

    def _record(self):
        return self._head() + [len(self.a_terms), len(self.b_terms), 0]

    def _term_lists(self):
        return [self.a_terms, self.b_terms]

    def _terms(self):
        out = []
        for t in (t for terms in self._term_lists() for t in terms):
            sign, chal, col = t[0], t[1], t[2]
            off = t[3] if len(t) > 3 else 0
            if not -(1 << 31) <= int(off) < (1 << 31):
                raise ValueError(f"{type(self).__name__}: a term's offset is an int32")
            out.append([NONE if col is None else int(col), int(off), NONE if chal is None else int(chal), int(sign)])
        return out


class LogUpColumn(ExtColumn):
    """One running sum of fractions.  init, mask, inclusive: as for ExtColumn;  fractions: a list of (numerator_terms, denominator_terms) in
    ExtColumn's term tuples -- an empty numerator is the literal 1, a denominator has at least one term, and where a denominator is zero the
    fraction contributes nothing (inv(0) = 0).  No fraction at all: the column holds its init everywhere."""

    def __init__(self, init, fractions, mask=None, inclusive=False):
        self.init, self.fractions, self.mask, self.inclusive = init, [(list(nt), list(dt)) for nt, dt in fractions], mask, bool(inclusive)

    def _record(self):
        return self._head() + [len(self.fractions), 0, 0]

    def _fractions(self):
        return [[len(nt), len(dt)] for nt, dt in self.fractions]

    def _term_lists(self):
        return [terms for fraction in self.fractions for terms in fraction]


def _arguments(who, planner, base, challenges, columns, fq, out):
    cols = base.columns if isinstance(base, Matrix) else list(base)
    columns = list(columns)
    if not cols:
        raise ValueError(f"{who}: an empty base table")
    n, base_field = len(cols[0]), cols[0].field
    if any(len(c) != n or c.field != base_field for c in cols):
        raise ValueError(f"{who}: base columns of different lengths or fields")
    if challenges is not None and challenges.field != fq:
        raise ValueError(f"{who}: the challenges are not elements of `fq`")
    outs = [GpuVec(planner, n, fq) for _ in columns] if out is None else list(out)
    return cols, columns, n, base_field, outs


def _build_affine(planner, cols, n, base_field, challenges, columns, fq, outs):
    recs = np.array([c._record() for c in columns], dtype=np.int64).astype(np.int32)      # (na, nb, pad are uint32 of the same bits)
    terms = np.array([t for c in columns for t in c._terms()], dtype=np.int32).reshape(-1, 4)
    L = planner.lib
    L.check(L.ms_build_extension_columns(planner.handle, base_field, fq, n, _ptr_array(cols), len(cols),
                                         challenges.ptr if challenges is not None else None, len(challenges) if challenges is not None else 0,
                                         recs.ctypes.data, terms.ctypes.data if terms.size else None, len(columns), _ptr_array(outs)))


def _build_logup(planner, cols, n, base_field, challenges, columns, fq, outs):
    recs = np.array([c._record() for c in columns], dtype=np.int64).astype(np.int32)      # (nf and the pads are uint32 of the same bits)
    fracs = np.array([f for c in columns for f in c._fractions()], dtype=np.int64).astype(np.uint32).reshape(-1, 2)
    terms = np.array([t for c in columns for t in c._terms()], dtype=np.int32).reshape(-1, 4)
    L = planner.lib
    L.check(L.ms_build_logup_columns(planner.handle, base_field, fq, n, _ptr_array(cols), len(cols),
                                     challenges.ptr if challenges is not None else None, len(challenges) if challenges is not None else 0,
                                     recs.ctypes.data, fracs.ctypes.data if fracs.size else None, terms.ctypes.data if terms.size else None,
                                     len(columns), _ptr_array(outs)))


def build_extension_columns(planner, base, challenges, columns, fq, out=None):
    """-> Matrix of len(columns) columns of `fq`, as many rows as `base` (a Matrix of base-field columns, or a list of GpuVecs: the table
    is only pointers and need not be the committed trace).  challenges: GpuVec of `fq` elements (e.g. `PublicCoin.draw(fq, k)`), or None
    when no term and no init names one.  columns: ExtColumn and LogUpColumn records in any mix -- one ms_build_extension_columns call for
    the former, one ms_build_logup_columns call for the latter, the result in the order listed.  Enqueues and returns: no host wait."""
    cols, columns, n, base_field, outs = _arguments("build_extension_columns", planner, base, challenges, columns, fq, out)
    affine = [k for k, c in enumerate(columns) if not isinstance(c, LogUpColumn)]
    logup = [k for k, c in enumerate(columns) if isinstance(c, LogUpColumn)]
    if affine:
        _build_affine(planner, cols, n, base_field, challenges, [columns[k] for k in affine], fq, [outs[k] for k in affine])
    if logup:
        _build_logup(planner, cols, n, base_field, challenges, [columns[k] for k in logup], fq, [outs[k] for k in logup])
    return Matrix(outs)


def build_logup_columns(planner, base, challenges, columns, fq, out=None):
    """`build_extension_columns` for LogUpColumn records alone: ONE ms_build_logup_columns call (three launches however many columns)."""
    cols, columns, n, base_field, outs = _arguments("build_logup_columns", planner, base, challenges, columns, fq, out)
    if any(not isinstance(c, LogUpColumn) for c in columns):
        raise TypeError("build_logup_columns: every column is a LogUpColumn")
    if columns:
        _build_logup(planner, cols, n, base_field, challenges, columns, fq, outs)
    return Matrix(outs)


class LookupTuple:
    """One tuple of base columns: the table's columns, or one set of looked-up columns.  cols: 1 .. 4 indices into the base matrix;
    mask: None (every row is active), ("nonzero", m) or ("zero", m), as for ExtColumn."""

    def __init__(self, cols, mask=None):
        self.cols, self.mask = [int(c) for c in cols], mask
        if not 1 <= len(self.cols) <= LOOKUP_MAX_WIDTH:
            raise ValueError(f"LookupTuple: a tuple has 1 .. {LOOKUP_MAX_WIDTH} columns, not {len(self.cols)}")
        _mask_words("LookupTuple", mask)

    def _record(self):
        """the eight 32-bit words of ms_lookup_tuple: cols[4], mask, mask_col, pad0, pad1"""
        mask = _mask_words("LookupTuple", self.mask)
        return self.cols + [0] * (LOOKUP_MAX_WIDTH - len(self.cols)) + [mask[0], mask[1], 0, 0]


class LookupMissing(LookupError):
    """`LookupReport.check()`: a looked-up tuple is not a row of the table.  .set, .row, .values (canonical integers), .missing"""


class LookupReport:
    """What `lookup_multiplicities` found: the ms_lookup_report in device memory, downloaded (a host wait) when a field is first read.
    .missing: looked-up rows whose tuple the table does not hold; .first_missing_set / .first_missing_row: the smallest (set, row) among
    them (0, 0 when there is none); .duplicate_table_rows: active table rows equal to an earlier one (their m is 0)."""

    def __init__(self, planner, buf, cols, lookups):
        self.planner, self.buf, self._cols, self._lookups, self._rec = planner, buf, cols, lookups, None

    def _read(self):
        if self._rec is None:
            rec = LookupReportRecord()
            self.planner.lib.check(self.planner.lib.ms_download(self.planner.handle, ctypes.addressof(rec), self.buf.ptr, ctypes.sizeof(rec)))
            self._rec = rec
        return self._rec

    missing = property(lambda self: int(self._read().missing))
    first_missing_row = property(lambda self: int(self._read().first_missing_row))
    first_missing_set = property(lambda self: int(self._read().first_missing_set))
    duplicate_table_rows = property(lambda self: int(self._read().duplicate_table_rows))

    def __bool__(self):
        return self.missing == 0                 # true when every looked-up tuple was found

    def __repr__(self):
        return (f"LookupReport(missing={self.missing}, first_missing_set={self.first_missing_set}, first_missing_row={self.first_missing_row}, "
                f"duplicate_table_rows={self.duplicate_table_rows})")

    def first_missing_values(self):
        """the canonical values of the first missing tuple (it downloads those elements, nothing else), or None"""
        if not self.missing:
            return None
        row, L = self.first_missing_row, self.planner.lib
        vals = []
        for c in self._lookups[self.first_missing_set].cols:
            col = self._cols[c]
            V = FIELD_WORDS[col.field]
            w = np.empty(V, dtype=np.uint64)
            L.check(L.ms_download(self.planner.handle, w.ctypes.data, col.ptr + row * V * 8, V * 8))
            vals.append(gl_from_mont(int(w[0])) if col.field == GOLDILOCKS_FP else f252_from_mont_limbs([int(x) for x in w]))
        return vals

    def check(self):
        """raises LookupMissing, naming set, row and the tuple's values, when a looked-up tuple is not in the table"""
        if self.missing:
            s, row, vals = self.first_missing_set, self.first_missing_row, self.first_missing_values()
            err = LookupMissing(f"lookup set {s}, row {row}: the tuple ({', '.join(str(v) for v in vals)}) in base columns {self._lookups[s].cols} "
                                f"is not a row of the table; {self.missing} looked-up row(s) in all have no table row")
            err.set, err.row, err.values, err.missing = s, row, vals, self.missing
            raise err
        return self


def lookup_multiplicities(planner, base, table, lookups, out=None):
    """-> (m, report): m[j] = how many active rows of the `lookups` (LookupTuple records of one width) hold the tuple of row j of `table`
    (a LookupTuple), as elements of the base field; equal table rows: the first takes the credit.  base: a Matrix or a list of GpuVecs;
    out: the GpuVec to fill -- it may be a column of `base` that no tuple and no mask names, the trace's own m column -- or None for a new
    one.  report: a LookupReport.  Enqueues and returns: no host wait until the report is read."""
    cols = base.columns if isinstance(base, Matrix) else list(base)
    lookups = list(lookups)
    if not cols:
        raise ValueError("lookup_multiplicities: an empty base table")
    n, field = len(cols[0]), cols[0].field
    if any(len(c) != n or c.field != field for c in cols):
        raise ValueError("lookup_multiplicities: base columns of different lengths or fields")
    if any(len(t.cols) != len(table.cols) for t in lookups):
        raise ValueError("lookup_multiplicities: every lookup set has as many columns as the table")
    m = GpuVec(planner, n, field) if out is None else out
    if len(m) != n or m.field != field:
        raise ValueError("lookup_multiplicities: `out` is a column of the base field, as long as the base columns")
    buf = GpuVec(planner, ctypes.sizeof(LookupReportRecord) // 8, GOLDILOCKS_FP)
    trec = np.array(table._record(), dtype=np.int32)
    lrec = np.array([t._record() for t in lookups], dtype=np.int32).reshape(-1, 8)
    assert trec.nbytes == ctypes.sizeof(LookupTupleRecord)
    L = planner.lib
    L.check(L.ms_lookup_multiplicities(planner.handle, field, n, _ptr_array(cols), len(cols), len(table.cols), trec.ctypes.data,
                                       lrec.ctypes.data if lrec.size else None, len(lookups), m.ptr, buf.ptr))
    return m, LookupReport(planner, buf, cols, lookups)


class SortKey:
    """The key rows are sorted by: cols, 1 .. 4 indices into the base matrix, cols[0] the most significant; ascending, as canonical integers.
    mask: None (every row is active), ("nonzero", m) or ("zero", m), as for ExtColumn: inactive rows follow the sorted ones, in their order."""

    def __init__(self, cols, mask=None):
        self.cols, self.mask = [int(c) for c in cols], mask
        if not 1 <= len(self.cols) <= SORT_MAX_KEYS:
            raise ValueError(f"SortKey: a key has 1 .. {SORT_MAX_KEYS} columns, not {len(self.cols)}")
        _mask_words("SortKey", mask)

    def _record(self):
        """the eight 32-bit words of ms_sort_key: cols[4], mask, mask_col, pad0, pad1"""
        mask = _mask_words("SortKey", self.mask)
        return self.cols + [0] * (SORT_MAX_KEYS - len(self.cols)) + [mask[0], mask[1], 0, 0]


class DeviceIndex(DeviceBytes):
    """n 32-bit row indices in device memory: the permutation `sort_rows` writes and `permute_columns` reads."""

    def __init__(self, planner, n):
        super().__init__(planner, 4 * n)
        self.n = n

    @classmethod
    def from_numpy(cls, planner, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32).ravel()
        v = cls(planner, arr.size)
        if arr.size:
            planner.lib.check(planner.lib.ms_upload(planner.handle, v.ptr, arr.ctypes.data, arr.nbytes))
        return v

    def to_numpy(self, n=None):
        """the first n indices (default: all) on the host, as uint32 (a host wait)"""
        return super().to_numpy(4 * (self.n if n is None else n)).view(np.uint32)

    def __len__(self):
        return self.n


class SortReport:
    """What `sort_rows` found: the ms_sort_report in device memory, downloaded (a host wait) when a field is first read.
    .active: the rows the mask lets through (the sorted head of the permutation); .varying_bytes: the (component, byte) positions at which
    two active rows differ -- the number of radix passes the call executed."""

    def __init__(self, planner, buf):
        self.planner, self.buf, self._rec = planner, buf, None

    def _read(self):
        if self._rec is None:
            rec = SortReportRecord()
            self.planner.lib.check(self.planner.lib.ms_download(self.planner.handle, ctypes.addressof(rec), self.buf.ptr, ctypes.sizeof(rec)))
            self._rec = rec
        return self._rec

    active = property(lambda self: int(self._read().active))
    varying_bytes = property(lambda self: int(self._read().varying_bytes))

    def __repr__(self):
        return f"SortReport(active={self.active}, varying_bytes={self.varying_bytes})"


def _same_columns(what, cols):
    if not cols:
        raise ValueError(f"{what}: no columns")
    n, field = len(cols[0]), cols[0].field
    if any(len(c) != n or c.field != field for c in cols):
        raise ValueError(f"{what}: columns of different lengths or fields")
    return n, field


def sort_rows(planner, base, key, n=None):
    """-> (perm, report): perm, a DeviceIndex of n uint32, lists the active rows of `base` (a Matrix or a list of GpuVecs) in ascending order
    of `key` (a SortKey) -- rows of equal keys in their original order -- and then the inactive rows in their original order.  n: sort the
    first n rows only (default: all).  report: a SortReport.  Enqueues and returns: no host wait until the report or the index is read."""
    cols = base.columns if isinstance(base, Matrix) else list(base)
    rows, field = _same_columns("sort_rows", cols)
    n = rows if n is None else int(n)
    if not 0 <= n <= rows:
        raise ValueError(f"sort_rows: {n} rows of columns that hold {rows}")
    perm = DeviceIndex(planner, n)
    buf = GpuVec(planner, ctypes.sizeof(SortReportRecord) // 8, GOLDILOCKS_FP)
    rec = np.array(key._record(), dtype=np.int32)
    assert rec.nbytes == ctypes.sizeof(SortKeyRecord)
    L = planner.lib
    L.check(L.ms_sort_rows(planner.handle, field, n, _ptr_array(cols), len(cols), len(key.cols), rec.ctypes.data, perm.ptr, buf.ptr))
    return perm, SortReport(planner, buf)


def permute_columns(planner, columns, index, n_out=None, out=None):
    """-> a Matrix with out[c][i] = columns[c][index[i]] for i < n_out (a zero element where index[i] is not a row of `columns`).
    columns: a Matrix or a list of GpuVecs of one field, at most 128; index: a DeviceIndex (or DeviceBytes holding uint32); n_out: how many
    entries of it to use (default: all); out: GpuVecs of at least n_out elements to fill (their first n_out), or None for new ones."""
    cols = columns.columns if isinstance(columns, Matrix) else list(columns)
    n_src, field = _same_columns("permute_columns", cols)
    held = index.nbytes // 4
    n_out = held if n_out is None else int(n_out)
    if not 0 <= n_out <= held:
        raise ValueError(f"permute_columns: {n_out} entries of an index that holds {held}")
    if out is None:
        outs = [GpuVec(planner, n_out, field) for _ in cols]
    else:
        outs = out.columns if isinstance(out, Matrix) else list(out)
        if len(outs) != len(cols) or any(len(o) < n_out or o.field != field for o in outs):
            raise ValueError("permute_columns: `out` is one column per source column, of its field, of at least n_out elements")
    L = planner.lib
    L.check(L.ms_permute_columns(planner.handle, field, n_src, _ptr_array(cols), _ptr_array(outs), len(cols), index.ptr, n_out))
    return Matrix(outs)


class JoinReport:
    """What `join_rows` found: the ms_join_report in device memory, downloaded (a host wait) when a field is first read.
    .matched: active rows whose key the table holds; .missing: active rows whose key it does not; .first_missing_set / .first_missing_row:
    the smallest (set, row) among them (0, 0 when there is none); .duplicate_table_rows: active table rows equal to an earlier one (no row
    matches them); .table_active: the table rows its mask lets through."""

    def __init__(self, planner, buf, cols, keys):
        self.planner, self.buf, self._cols, self._keys, self._rec = planner, buf, cols, keys, None

    def _read(self):
        if self._rec is None:
            rec = JoinReportRecord()
            self.planner.lib.check(self.planner.lib.ms_download(self.planner.handle, ctypes.addressof(rec), self.buf.ptr, ctypes.sizeof(rec)))
            self._rec = rec
        return self._rec

    matched = property(lambda self: int(self._read().matched))
    missing = property(lambda self: int(self._read().missing))
    first_missing_row = property(lambda self: int(self._read().first_missing_row))
    first_missing_set = property(lambda self: int(self._read().first_missing_set))
    duplicate_table_rows = property(lambda self: int(self._read().duplicate_table_rows))
    table_active = property(lambda self: int(self._read().table_active))

    def __bool__(self):
        return self.missing == 0                 # true when every active row found its table row

    def __repr__(self):
        return (f"JoinReport(matched={self.matched}, missing={self.missing}, first_missing_set={self.first_missing_set}, "
                f"first_missing_row={self.first_missing_row}, duplicate_table_rows={self.duplicate_table_rows}, table_active={self.table_active})")

    def first_missing_values(self):
        """the canonical values of the first missing key (it downloads those elements, nothing else), or None"""
        if not self.missing:
            return None
        row, L = self.first_missing_row, self.planner.lib
        vals = []
        for c in self._keys[self.first_missing_set].cols:
            col = self._cols[c]
            V = FIELD_WORDS[col.field]
            w = np.empty(V, dtype=np.uint64)
            L.check(L.ms_download(self.planner.handle, w.ctypes.data, col.ptr + row * V * 8, V * 8))
            vals.append(gl_from_mont(int(w[0])) if col.field == GOLDILOCKS_FP else f252_from_mont_limbs([int(x) for x in w]))
        return vals

    def check(self):
        """raises LookupMissing, naming set, row and the key's values, when an active row's key is not in the table"""
        if self.missing:
            s, row, vals = self.first_missing_set, self.first_missing_row, self.first_missing_values()
            err = LookupMissing(f"key set {s}, row {row}: the key ({', '.join(str(v) for v in vals)}) in base columns {self._keys[s].cols} "
                                f"is not a row of the table; {self.missing} row(s) in all have no table row")
            err.set, err.row, err.values, err.missing = s, row, vals, self.missing
            raise err
        return self


def join_rows(planner, table, table_key, base, keys):
    """-> (matches, report): matches[s][i] = the smallest active row of `table` whose key (`table_key`, a LookupTuple over `table`) equals
    the key of row i of `base` under keys[s] (LookupTuples of that width over `base`), or JOIN_NONE for an inactive row and for a key the
    table does not hold.  table, base: each a Matrix or a list of GpuVecs, of one length and one field, both of the same field (they may be
    the same columns: a self-join).  matches: one DeviceIndex per set, which `permute_columns` reads as it is.  report: a JoinReport.
    Enqueues and returns: no host wait until the report or an index is read."""
    tcols = table.columns if isinstance(table, Matrix) else list(table)
    cols = base.columns if isinstance(base, Matrix) else list(base)
    keys = list(keys)
    n_table, field = _same_columns("join_rows: table", tcols)
    n, base_field = _same_columns("join_rows: base", cols)
    if base_field != field:
        raise ValueError("join_rows: the table and the base columns are of different fields")
    if any(len(k.cols) != len(table_key.cols) for k in keys):
        raise ValueError("join_rows: every key set has as many columns as the table key")
    if len(keys) > JOIN_MAX_SETS:
        raise ValueError(f"join_rows: at most {JOIN_MAX_SETS} key sets in one call, not {len(keys)}")
    matches = [DeviceIndex(planner, n) for _ in keys]
    buf = GpuVec(planner, ctypes.sizeof(JoinReportRecord) // 8, GOLDILOCKS_FP)
    trec = np.array(table_key._record(), dtype=np.int32)
    krec = np.array([k._record() for k in keys], dtype=np.int32).reshape(-1, 8)
    assert trec.nbytes == ctypes.sizeof(LookupTupleRecord)
    L = planner.lib
    L.check(L.ms_join_rows(planner.handle, field, n_table, _ptr_array(tcols), len(tcols), trec.ctypes.data, n, _ptr_array(cols), len(cols),
                           len(table_key.cols), krec.ctypes.data if krec.size else None, len(keys), _ptr_array(matches) if matches else None, buf.ptr))
    return matches, JoinReport(planner, buf, cols, keys)


def fetch_columns(planner, table, table_key, base, key, payload, out=None, check=False):
    """-> (Matrix, report): for every row of `base`, the `payload` columns (indices into `table`) of the table row that holds its key:
    `join_rows` for the one set `key`, then `permute_columns` by the match.  A row that is inactive or whose key the table does not hold
    gets zero elements (the report counts the latter).  out: GpuVecs to fill, one per payload column, or None for new ones.  check: read the
    report (a host wait) and raise LookupMissing if a key is missing."""
    tcols = table.columns if isinstance(table, Matrix) else list(table)
    payload = [int(c) for c in payload]
    if not payload or any(not 0 <= c < len(tcols) for c in payload):
        raise ValueError(f"fetch_columns: payload is a non-empty list of indices into the table's {len(tcols)} columns, not {payload!r}")
    (match,), report = join_rows(planner, tcols, table_key, base, [key])
    fetched = permute_columns(planner, [tcols[c] for c in payload], match, out=out)
    if check:
        report.check()
    return fetched, report


def _canonical_at(planner, col, row):
    """the canonical integer of element `row` of a base column (it downloads that element, nothing else)"""
    V = FIELD_WORDS[col.field]
    w = np.empty(V, dtype=np.uint64)
    planner.lib.check(planner.lib.ms_download(planner.handle, w.ctypes.data, col.ptr + row * V * 8, V * 8))
    return gl_from_mont(int(w[0])) if col.field == GOLDILOCKS_FP else f252_from_mont_limbs([int(x) for x in w])


class LimbSpec:
    """One decomposition: base column `src` -> the `nlimbs` columns dst0 .. dst0 + nlimbs - 1, limb j the bits [j * bits, (j + 1) * bits) of
    the value's canonical integer.  mask: None (every row is active), ("nonzero", m) or ("zero", m), as for ExtColumn: an inactive row gets
    zero limbs."""

    def __init__(self, src, dst0, nlimbs, bits, mask=None):
        self.src, self.dst0, self.nlimbs, self.bits, self.mask = int(src), int(dst0), int(nlimbs), int(bits), mask
        if not 1 <= self.bits <= RANGE_MAX_LIMB_BITS:
            raise ValueError(f"LimbSpec: a limb has 1 .. {RANGE_MAX_LIMB_BITS} bits, not {self.bits}")
        if not 1 <= self.nlimbs <= RANGE_MAX_LIMBS:
            raise ValueError(f"LimbSpec: 1 .. {RANGE_MAX_LIMBS} limbs, not {self.nlimbs}")
        _mask_words("LimbSpec", mask)

    def _record(self):
        """the eight 32-bit words of ms_limb_spec: src, dst0, nlimbs, bits, mask, mask_col, pad0, pad1"""
        mask = _mask_words("LimbSpec", self.mask)
        return [self.src, self.dst0, self.nlimbs, self.bits, mask[0], mask[1], 0, 0]


class RangeSet:
    """One looked-up column of a range check: base column `col`; mask as for ExtColumn."""

    def __init__(self, col, mask=None):
        self.col, self.mask = int(col), mask
        self.cols = [self.col]
        _mask_words("RangeSet", mask)

    def _record(self):
        """the four 32-bit words of ms_range_set: col, mask, mask_col, pad"""
        mask = _mask_words("RangeSet", self.mask)
        return [self.col, mask[0], mask[1], 0]


class LimbReport:
    """What `limb_decompose` found: the ms_limb_report in device memory, downloaded (a host wait) when a field is first read.
    .overflow: active rows whose value does not fit nlimbs * bits bits (they still got their low limbs); .first_overflow_spec /
    .first_overflow_row: the smallest (spec, row) among them (0, 0 when there is none); .active: the rows the masks let through, over all
    specs."""

    def __init__(self, planner, buf, cols, specs):
        self.planner, self.buf, self._cols, self._specs, self._rec = planner, buf, cols, specs, None

    def _read(self):
        if self._rec is None:
            rec = LimbReportRecord()
            self.planner.lib.check(self.planner.lib.ms_download(self.planner.handle, ctypes.addressof(rec), self.buf.ptr, ctypes.sizeof(rec)))
            self._rec = rec
        return self._rec

    overflow = property(lambda self: int(self._read().overflow))
    first_overflow_row = property(lambda self: int(self._read().first_overflow_row))
    first_overflow_spec = property(lambda self: int(self._read().first_overflow_spec))
    active = property(lambda self: int(self._read().active))

    def __bool__(self):
        return self.overflow == 0                # true when every value fits its limbs

    def __repr__(self):
        return (f"LimbReport(overflow={self.overflow}, first_overflow_spec={self.first_overflow_spec}, first_overflow_row={self.first_overflow_row}, "
                f"active={self.active})")

    def first_overflow_value(self):
        """the canonical value of the first overflowing row (it downloads that element, nothing else), or None"""
        if not self.overflow:
            return None
        return _canonical_at(self.planner, self._cols[self._specs[self.first_overflow_spec].src], self.first_overflow_row)

    def check(self):
        """raises LookupMissing, naming spec, row and the value, when a value does not fit its limbs"""
        if self.overflow:
            k, row, v = self.first_overflow_spec, self.first_overflow_row, self.first_overflow_value()
            spec = self._specs[k]
            err = LookupMissing(f"limb spec {k}, row {row}: the value {v} in base column {spec.src} does not fit {spec.nlimbs} limb(s) of {spec.bits} bits; "
                                f"{self.overflow} row(s) in all do not fit")
            err.set, err.spec, err.row, err.values, err.value, err.missing = k, k, row, [v], v, self.overflow
            raise err
        return self


class RangeReport(LookupReport):
    """What `range_multiplicities` found: a LookupReport (duplicate_table_rows is 0: the table 0 .. 2^bits - 1 has none) whose check()
    names the set, the row and the value that is not below 2^bits."""

    def __init__(self, planner, buf, cols, sets, bits):
        super().__init__(planner, buf, cols, sets)
        self.bits = bits

    def __repr__(self):
        return f"RangeReport(missing={self.missing}, first_missing_set={self.first_missing_set}, first_missing_row={self.first_missing_row})"

    def check(self):
        if self.missing:
            s, row, vals = self.first_missing_set, self.first_missing_row, self.first_missing_values()
            err = LookupMissing(f"range set {s}, row {row}: the value {vals[0]} in base column {self._lookups[s].col} is not below 2^{self.bits}; "
                                f"{self.missing} looked-up row(s) in all are out of range")
            err.set, err.row, err.values, err.missing = s, row, vals, self.missing
            raise err
        return self


def _write_spec_columns(who, planner, trace, specs, max_specs, record, refuse):
    """What limb_decompose and bitwise_columns share: the trace's columns and field, the limit on the specs, refuse(spec, field) -> why the
    field does not take the spec (or None), the specs as `record`s, the report buffer, the call ms_<who> -> (report buffer, columns, specs)"""
    cols = trace.columns if isinstance(trace, Matrix) else list(trace)
    specs = list(specs)
    n, field = _same_columns(who, cols)
    if field not in (GOLDILOCKS_FP, STARK252_FP):
        raise ValueError(f"{who}: the trace is over Fp or Fp252")
    if len(specs) > max_specs:
        raise ValueError(f"{who}: at most {max_specs} specs in one call, not {len(specs)}")
    for k, sp in enumerate(specs):
        why = refuse(sp, field)
        if why:
            raise ValueError(f"{who}: spec {k}: {why}")
    buf = GpuVec(planner, ctypes.sizeof(LimbReportRecord) // 8, GOLDILOCKS_FP)
    rec = np.array([sp._record() for sp in specs], dtype=np.int32).reshape(-1, 8)
    assert rec.nbytes == len(specs) * ctypes.sizeof(record)
    L = planner.lib
    L.check(getattr(L, "ms_" + who)(planner.handle, field, n, _ptr_array(cols), len(cols), rec.ctypes.data if rec.size else None, len(specs), buf.ptr))
    return buf, cols, specs


def _multiplicity_buffers(who, planner, n, field, T, rows, sets, record, out, n_m):
    """What range_multiplicities and bitwise_multiplicities share: n_m (default: the length of `out`, or n) against the table's T rows
    (`rows` in the refusal's words), the column m, the report buffer, the sets as `record`s -> (n_m, m, report buffer, records, their address)"""
    if n_m is None:
        n_m = len(out) if out is not None else n
    n_m = int(n_m)
    if n_m < T:
        raise ValueError(f"{who}: m holds {n_m} elements, fewer than the {rows} rows of the table")
    m = GpuVec(planner, n_m, field) if out is None else out
    if len(m) < n_m or m.field != field:
        raise ValueError(f"{who}: `out` is a column of the base field of at least n_m elements")
    buf = GpuVec(planner, ctypes.sizeof(LookupReportRecord) // 8, GOLDILOCKS_FP)
    rec = np.array([s._record() for s in sets], dtype=np.int32).reshape(-1, ctypes.sizeof(record) // 4)
    assert rec.nbytes == len(sets) * ctypes.sizeof(record)
    return n_m, m, buf, rec, rec.ctypes.data if rec.size else None


def limb_decompose(planner, trace, specs):
    """Writes the limb columns of every LimbSpec into `trace` (a Matrix or a list of GpuVecs of one length and field) -> a LimbReport.
    The destination columns of a spec are columns of the trace that no spec reads (as source or mask) and no other spec writes.
    Enqueues and returns: no host wait until the report is read."""
    def too_wide(sp, field):
        if sp.nlimbs * sp.bits > 64 * FIELD_WORDS[field]:
            return f"{sp.nlimbs} limbs of {sp.bits} bits are more than the {64 * FIELD_WORDS[field]} bits of an element's words"
    return LimbReport(planner, *_write_spec_columns("limb_decompose", planner, trace, specs, RANGE_MAX_SPECS, LimbSpecRecord, too_wide))


def range_multiplicities(planner, trace, bits, sets, out=None, n_m=None):
    """-> (m, report): m[j] = how many active rows of the `sets` (RangeSet records) hold the value j, for j < 2^bits, and zero from there to
    n_m (default: the length of `out`, or of the trace), as elements of the base field.  out: the GpuVec to fill (its first n_m elements)
    -- it may be a column of `trace` that no set and no mask names, the trace's own m column -- or None for a new one.  report: a
    RangeReport; a value that is not below 2^bits is counted there as missing.  Enqueues and returns: no host wait until it is read."""
    cols = trace.columns if isinstance(trace, Matrix) else list(trace)
    sets, bits = list(sets), int(bits)
    n, field = _same_columns("range_multiplicities", cols)
    if not 1 <= bits <= RANGE_MAX_TABLE_BITS:
        raise ValueError(f"range_multiplicities: bits is 1 .. {RANGE_MAX_TABLE_BITS}, not {bits}")
    if len(sets) > RANGE_MAX_SETS:
        raise ValueError(f"range_multiplicities: at most {RANGE_MAX_SETS} sets in one call, not {len(sets)}")
    n_m, m, buf, rec, h_sets = _multiplicity_buffers("range_multiplicities", planner, n, field, 1 << bits, f"2^{bits}", sets, RangeSetRecord, out, n_m)
    L = planner.lib
    L.check(L.ms_range_multiplicities(planner.handle, field, n, _ptr_array(cols), len(cols), bits, h_sets, len(sets), n_m, m.ptr, buf.ptr))
    return m, RangeReport(planner, buf, cols, sets, bits)


def _bitwise_op(who, op):
    """"and" | "or" | "xor" | 0 | 1 | 2 -> the op code"""
    code = BITWISE_OPS.get(op, op) if isinstance(op, str) else op
    if code not in (0, 1, 2):
        raise ValueError(f"{who}: op is 'and', 'or' or 'xor' (0, 1, 2), not {op!r}")
    return int(code)


def bitwise_apply(op, x, y):
    """x op y on Python integers, op a code or a name"""
    code = _bitwise_op("bitwise_apply", op)
    return x & y if code == 0 else x | y if code == 1 else x ^ y


class BitwiseSpec:
    """One result column: base column `dst` = (a mod 2^width) op (b mod 2^width) on the canonical integers of base columns `a` and `b`
    (a == b is allowed); op "and", "or", "xor".  mask: None, ("nonzero", m) or ("zero", m), as for ExtColumn: an inactive row gets zero."""

    def __init__(self, op, a, b, dst, width, mask=None):
        self.op, self.a, self.b, self.dst, self.width, self.mask = _bitwise_op("BitwiseSpec", op), int(a), int(b), int(dst), int(width), mask
        if not 1 <= self.width <= max(BITWISE_WMAX.values()):
            raise ValueError(f"BitwiseSpec: an operand has 1 .. {max(BITWISE_WMAX.values())} bits, not {self.width}")
        _mask_words("BitwiseSpec", mask)

    def _record(self):
        """the eight 32-bit words of ms_bitwise_spec: op, a, b, dst, width, mask, mask_col, pad"""
        mask = _mask_words("BitwiseSpec", self.mask)
        return [self.op, self.a, self.b, self.dst, self.width, mask[0], mask[1], 0]


class BitwiseSet:
    """One looked-up operation of a bitwise check: the `nlimbs` limb pairs of base columns `a` and `b` under `op`, and the result column `c`
    to check against a op b (None: there is none).  mask as for ExtColumn."""

    def __init__(self, op, a, b, c, nlimbs, mask=None):
        self.op, self.a, self.b, self.c, self.nlimbs, self.mask = _bitwise_op("BitwiseSet", op), int(a), int(b), None if c is None else int(c), int(nlimbs), mask
        if self.c is not None and self.c < 0:
            raise ValueError(f"BitwiseSet: c is a column index or None, not {c}")
        if not 1 <= self.nlimbs <= BITWISE_MAX_LIMBS:
            raise ValueError(f"BitwiseSet: 1 .. {BITWISE_MAX_LIMBS} limbs, not {self.nlimbs}")
        self.cols = [self.a, self.b] + ([] if self.c is None else [self.c])
        _mask_words("BitwiseSet", mask)

    def _record(self):
        """the eight 32-bit words of ms_bitwise_set: op, a, b, c, nlimbs, mask, mask_col, pad"""
        mask = _mask_words("BitwiseSet", self.mask)
        return [self.op, self.a, self.b, -1 if self.c is None else self.c, self.nlimbs, mask[0], mask[1], 0]


class BitwiseColumnsReport(LimbReport):
    """What `bitwise_columns` found: a LimbReport whose overflow counts the active rows with an operand that does not fit `width` bits."""

    def first_overflow_value(self):
        """the canonical values (a, b) of the first overflowing row (it downloads those two elements, nothing else), or None"""
        if not self.overflow:
            return None
        spec, row = self._specs[self.first_overflow_spec], self.first_overflow_row
        return (_canonical_at(self.planner, self._cols[spec.a], row), _canonical_at(self.planner, self._cols[spec.b], row))

    def check(self):
        """raises LookupMissing, naming spec, row and both operands, when an operand does not fit its width"""
        if self.overflow:
            k, row, v = self.first_overflow_spec, self.first_overflow_row, self.first_overflow_value()
            spec = self._specs[k]
            err = LookupMissing(f"bitwise spec {k}, row {row}: the operands {v[0]} and {v[1]} in base columns {spec.a} and {spec.b} do not both fit {spec.width} bits; "
                                f"{self.overflow} row(s) in all do not fit")
            err.set, err.spec, err.row, err.values, err.missing = k, k, row, list(v), self.overflow
            raise err
        return self


class BitwiseReport(LookupReport):
    """What `bitwise_multiplicities` found: a LookupReport (duplicate_table_rows is 0) whose check() names the set, the row and the three
    canonical values a, b, c of the first row that is not in the table: an operand past its limbs, or c != a op b."""

    def __init__(self, planner, buf, cols, sets, bits):
        super().__init__(planner, buf, cols, sets)
        self.bits = bits

    def __repr__(self):
        return f"BitwiseReport(missing={self.missing}, first_missing_set={self.first_missing_set}, first_missing_row={self.first_missing_row})"

    def first_missing_values(self):
        """[a, b, c] of the first missing row as canonical integers (it downloads those elements, nothing else), c = a op b where the set
        has no result column; or None"""
        vals = super().first_missing_values()
        if vals is not None and len(vals) == 2:
            vals.append(bitwise_apply(self._lookups[self.first_missing_set].op, vals[0], vals[1]))
        return vals

    def check(self):
        if self.missing:
            s, row, vals = self.first_missing_set, self.first_missing_row, self.first_missing_values()
            st = self._lookups[s]
            name = {v: k for k, v in BITWISE_OPS.items()}[st.op]
            err = LookupMissing(f"bitwise set {s}, row {row}: a = {vals[0]}, b = {vals[1]}, c = {vals[2]} in base columns {st.a}, {st.b}, {st.c}: an operand is not below "
                                f"2^{st.nlimbs * self.bits} ({st.nlimbs} limbs of {self.bits} bits) or c is not a {name} b; {self.missing} looked-up row(s) in all are not in the table")
            err.set, err.row, err.values, err.missing = s, row, vals, self.missing
            raise err
        return self


def bitwise_columns(planner, trace, specs):
    """Writes the result column of every BitwiseSpec into `trace` (a Matrix or a list of GpuVecs of one length and field) -> a LimbReport
    (its overflow: active rows with an operand that does not fit `width` bits; their low bits still go into the result).  The dst of a spec
    is a column of the trace that no spec reads (as operand or mask) and no other spec writes.  Enqueues and returns: no host wait until the
    report is read."""
    def too_wide(sp, field):
        if sp.width > BITWISE_WMAX[field]:
            return f"an operand of this field has 1 .. {BITWISE_WMAX[field]} bits, not {sp.width}"
    return BitwiseColumnsReport(planner, *_write_spec_columns("bitwise_columns", planner, trace, specs, BITWISE_MAX_SPECS, BitwiseSpecRecord, too_wide))


def _bitwise_ops(who, bits, ops):
    bits, codes = int(bits), [_bitwise_op(who, op) for op in ops]
    if not 1 <= bits <= BITWISE_MAX_BITS:
        raise ValueError(f"{who}: bits is 1 .. {BITWISE_MAX_BITS}, not {bits}")
    if not 1 <= len(codes) <= BITWISE_MAX_OPS or len(set(codes)) != len(codes):
        raise ValueError(f"{who}: 1 .. {BITWISE_MAX_OPS} distinct ops, not {list(ops)!r}")
    T = len(codes) << (2 * bits)
    if T > 1 << BITWISE_MAX_TABLE_LOG:
        raise ValueError(f"{who}: {len(codes)} ops over pairs of {bits}-bit limbs are {T} table rows (at most 2^{BITWISE_MAX_TABLE_LOG})")
    return bits, np.array(codes, dtype=np.int32), T


def bitwise_table(planner, field, bits, ops, n_t=None, out=None, with_op=None):
    """-> [top, tx, ty, tz] (top is None without an op column): the table (op, x, y, x op y) over all pairs of `bits`-bit limbs, op by op in
    the order of `ops`, x the slower index, padded to n_t rows (default: the table's own len(ops) * 4^bits) by repeating the last row.
    out: the four GpuVecs to fill, [top or None, tx, ty, tz], or None for new ones; with_op: write the op column (default: when there is
    more than one op).  Enqueues and returns."""
    bits, codes, T = _bitwise_ops("bitwise_table", bits, ops)
    if field not in BITWISE_WMAX:
        raise ValueError("bitwise_table: the table is over Fp or Fp252")
    if out is not None:
        out = list(out)
        if len(out) != 4 or any(c is None for c in out[1:]):
            raise ValueError("bitwise_table: out is [top or None, tx, ty, tz]")
    if n_t is None:
        n_t = min(len(c) for c in out if c is not None) if out is not None else T
    n_t = int(n_t)
    if n_t < T:
        raise ValueError(f"bitwise_table: the columns hold {n_t} elements, fewer than the {T} rows of the table")
    if out is None:
        with_op = len(codes) > 1 if with_op is None else with_op
        out = [GpuVec(planner, n_t, field) if with_op else None] + [GpuVec(planner, n_t, field) for _ in range(3)]
    if any(c is not None and (len(c) < n_t or c.field != field) for c in out):
        raise ValueError("bitwise_table: `out` holds columns of `field` of at least n_t elements")
    L = planner.lib
    L.check(L.ms_bitwise_table(planner.handle, field, bits, codes.ctypes.data, len(codes), n_t, out[0].ptr if out[0] is not None else None, out[1].ptr, out[2].ptr, out[3].ptr))
    return out


def bitwise_multiplicities(planner, trace, bits, ops, sets, out=None, n_m=None):
    """-> (m, report): m[slot * 4^bits + (x << bits) + y] = how many limb pairs (x, y) the active, valid rows of the `sets` (BitwiseSet
    records) of the op at position `slot` of `ops` hold, and zero from len(ops) * 4^bits to n_m (default: the length of `out`, or of the
    trace), as elements of the base field -- the multiplicities of `bitwise_table`'s rows.  out: the GpuVec to fill (its first n_m elements)
    -- it may be a column of `trace` that no set and no mask names -- or None for a new one.  report: a BitwiseReport; a row with an
    operand not below 2^(nlimbs * bits), or whose c is not a op b, is counted there as missing and none of its limbs is counted.
    Enqueues and returns: no host wait until it is read."""
    cols = trace.columns if isinstance(trace, Matrix) else list(trace)
    sets = list(sets)
    n, field = _same_columns("bitwise_multiplicities", cols)
    bits, codes, T = _bitwise_ops("bitwise_multiplicities", bits, ops)
    if field not in BITWISE_WMAX:
        raise ValueError("bitwise_multiplicities: the trace is over Fp or Fp252")
    if len(sets) > BITWISE_MAX_SETS:
        raise ValueError(f"bitwise_multiplicities: at most {BITWISE_MAX_SETS} sets in one call, not {len(sets)}")
    for s, st in enumerate(sets):
        if st.op not in codes:
            raise ValueError(f"bitwise_multiplicities: set {s}: its op is not one of the table's ops")
        if st.nlimbs * bits > BITWISE_WMAX[field]:
            raise ValueError(f"bitwise_multiplicities: set {s}: {st.nlimbs} limbs of {bits} bits are more than the {BITWISE_WMAX[field]} bits an operand may have")
    n_m, m, buf, rec, h_sets = _multiplicity_buffers("bitwise_multiplicities", planner, n, field, T, T, sets, BitwiseSetRecord, out, n_m)
    L = planner.lib
    L.check(L.ms_bitwise_multiplicities(planner.handle, field, n, _ptr_array(cols), len(cols), bits, codes.ctypes.data, len(codes), h_sets, len(sets),
                                        n_m, m.ptr, buf.ptr))
    return m, BitwiseReport(planner, buf, cols, sets, bits)


GAP_MAX_GROUP, GAP_MAX_COLUMNS = 3, 128
_GAP_KIND = {"copy": 0, "zero": 1, "counter": 2, "flag": 3}


class GapSpec:
    """Which rows a derived table takes and where rows are inserted (ms_gap_spec).  group: 0 .. 3 indices into the base matrix -- a gap is
    only looked for between two consecutive rows that agree on them; counter: the index of the clock column, or None for no gaps (a plain
    stable select, or plain padding); mask: None, ("nonzero", m) or ("zero", m), as for SortKey."""

    def __init__(self, group=(), counter=None, mask=None):
        self.group, self.counter, self.mask = [int(c) for c in group], None if counter is None else int(counter), mask
        if len(self.group) > GAP_MAX_GROUP:
            raise ValueError(f"GapSpec: a group has 0 .. {GAP_MAX_GROUP} columns, not {len(self.group)}")
        if self.counter is not None and self.counter < 0:
            raise ValueError(f"GapSpec: counter is a column index or None, not {counter!r}")
        _mask_words("GapSpec", mask)

    def _record(self):
        """the eight 32-bit words of ms_gap_spec: group[3], ngroup, counter, mask, mask_col, pad0"""
        mask = _mask_words("GapSpec", self.mask)
        return self.group + [0] * (GAP_MAX_GROUP - len(self.group)) + [len(self.group), NONE if self.counter is None else self.counter, mask[0], mask[1], 0]


class GapError(ValueError):
    """`GapReport.check`: the counter does not ascend inside a group, or a gap was clipped."""


class GapReport:
    """What `gap_plan` found: the ms_gap_report in device memory, downloaded (a host wait) when a field is first read.
    .active: the positions the mask lets through; .rows_out: the rows of the derived table before padding; .gaps: the positions a dummy row
    follows; .max_gap: the longest run of dummy rows; .unordered / .first_unordered: positions whose counter does not ascend to the next
    row of their group (first_unordered is None when there is none); .saturated: gaps clipped at 2^32."""

    def __init__(self, planner, buf):
        self.planner, self.buf, self._rec = planner, buf, None

    def _read(self):
        if self._rec is None:
            rec = GapReportRecord()
            self.planner.lib.check(self.planner.lib.ms_download(self.planner.handle, ctypes.addressof(rec), self.buf.ptr, ctypes.sizeof(rec)))
            self._rec = rec
        return self._rec

    active = property(lambda self: int(self._read().active))
    rows_out = property(lambda self: int(self._read().rows_out))
    gaps = property(lambda self: int(self._read().gaps))
    max_gap = property(lambda self: int(self._read().max_gap))
    unordered = property(lambda self: int(self._read().unordered))
    saturated = property(lambda self: int(self._read().saturated))

    @property
    def first_unordered(self):
        v = int(self._read().first_unordered)
        return None if v == (1 << 64) - 1 else v

    def check(self):
        """raises GapError when the derived table is not the one the host loop builds: -> self otherwise"""
        if self.unordered:
            raise GapError(f"gap_plan: at {self.unordered} positions the counter does not ascend to the next row of the group, the first at {self.first_unordered}")
        if self.saturated:
            raise GapError(f"gap_plan: {self.saturated} gaps are longer than 2^32 rows and were clipped")
        return self

    def __repr__(self):
        return (f"GapReport(active={self.active}, rows_out={self.rows_out}, gaps={self.gaps}, max_gap={self.max_gap}, unordered={self.unordered}, "
                f"first_unordered={self.first_unordered}, saturated={self.saturated})")


class GapPlan:
    """What `gap_plan` returns and `gap_fill` reads: .start, the n + 1 prefix sums in device memory (DeviceBytes, uint64); .report, a
    GapReport; .perm, the index the plan went through (or None); .n, its positions; .n_src, the rows of the base columns."""

    def __init__(self, start, report, perm, n, n_src, field):
        self.start, self.report, self.perm, self.n, self.n_src, self.field = start, report, perm, n, n_src, field

    def start_to_numpy(self):
        """the n + 1 entries of start on the host, as uint64 (a host wait)"""
        return self.start.to_numpy(8 * (self.n + 1)).view(np.uint64)


def gap_plan(planner, base, spec, perm=None, n=None):
    """-> a GapPlan: for each of the n positions of `perm` (a DeviceIndex such as `sort_rows` returns; None: the rows of `base` in their
    order), how many rows of the derived table it gives -- none if the mask of `spec` (a GapSpec) does not hold, else 1 plus the clock
    cycles missing up to the next position of the same group -- as prefix sums in device memory (ms_gap_plan).  n: the first n positions
    only (default: all).  Enqueues and returns: no host wait until the report is read."""
    cols = base.columns if isinstance(base, Matrix) else list(base)
    rows, field = _same_columns("gap_plan", cols)
    held = rows if perm is None else perm.nbytes // 4
    n = held if n is None else int(n)
    if not 0 <= n <= held:
        raise ValueError(f"gap_plan: {n} positions of {'columns' if perm is None else 'an index'} that hold{'' if perm is None else 's'} {held}")
    start = DeviceBytes(planner, 8 * (n + 1))
    buf = GpuVec(planner, ctypes.sizeof(GapReportRecord) // 8, GOLDILOCKS_FP)
    rec = np.array(spec._record(), dtype=np.int32)
    assert rec.nbytes == ctypes.sizeof(GapSpecRecord)
    L = planner.lib
    L.check(L.ms_gap_plan(planner.handle, field, rows, _ptr_array(cols), len(cols), rec.ctypes.data, None if perm is None else perm.ptr, n, start.ptr, buf.ptr))
    return GapPlan(start, GapReport(planner, buf), perm, n, rows, field)


def gap_fill(planner, base, plan, columns, n_out=None, out=None):
    """-> a Matrix of len(columns) columns of n_out rows: the derived table of `plan` (a GapPlan of the same `base`), padded (ms_gap_fill).
    Output row j comes from the position s that covers it, k = j - start[s] rows after it; rows past the table continue its last row.
    columns: ("copy", c): base column c at that position; ("zero", c): the same on the position's own row and zero on the k > 0 rows after
    it; ("counter", c): the same plus k; ("flag", None): 0 on the own row, 1 after.  n_out: the rows to write; default: the least power of
    two >= max(rows_out, 1), which reads the report (the only host wait).  out: GpuVecs of at least n_out elements to fill, or None."""
    cols = base.columns if isinstance(base, Matrix) else list(base)
    rows, field = _same_columns("gap_fill", cols)
    if rows != plan.n_src or field != plan.field:
        raise ValueError("gap_fill: the plan was made for other columns")
    columns = list(columns)
    if not 1 <= len(columns) <= GAP_MAX_COLUMNS:
        raise ValueError(f"gap_fill: 1 .. {GAP_MAX_COLUMNS} columns, not {len(columns)}")
    rec = []
    for col in columns:
        if len(col) != 2 or col[0] not in _GAP_KIND or (col[0] != "flag" and col[1] is None):
            raise ValueError(f"gap_fill: a column is ('copy', c), ('zero', c), ('counter', c) or ('flag', None), not {col!r}")
        rec += [_GAP_KIND[col[0]], 0 if col[0] == "flag" else int(col[1])]
    if n_out is None:
        n_out = 1
        while n_out < plan.report.rows_out:
            n_out *= 2
    n_out = int(n_out)
    if n_out < 0:
        raise ValueError(f"gap_fill: {n_out} output rows")
    if out is None:
        outs = [GpuVec(planner, n_out, field) for _ in columns]
    else:
        outs = out.columns if isinstance(out, Matrix) else list(out)
        if len(outs) != len(columns) or any(len(o) < n_out or o.field != field for o in outs):
            raise ValueError("gap_fill: `out` is one column per record, of the base columns' field, of at least n_out elements")
    rec = np.array(rec, dtype=np.int32)
    assert rec.nbytes == len(columns) * ctypes.sizeof(GapColumnRecord)
    L = planner.lib
    L.check(L.ms_gap_fill(planner.handle, field, rows, _ptr_array(cols), len(cols), None if plan.perm is None else plan.perm.ptr, plan.n, plan.start.ptr,
                          rec.ctypes.data, _ptr_array(outs), len(columns), n_out))
    return Matrix(outs)
