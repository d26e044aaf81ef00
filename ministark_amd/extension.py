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

`build_extension_columns` takes a list that mixes both kinds: one call of each, the columns returned in the order listed."""
import numpy as np

from .api import GpuVec, Matrix, _ptr_array

MAX_TERMS, MAX_COLUMNS, NONE = 8, 32, -1
ROWS_PER_WORKGROUP = 1024             # msext::ROWS (csrc/ext_kernels.h): the rows one workgroup scans; tests/test_ext_abi.py keeps the two equal
_INIT = {0: 0, 1: 1}
_MASK = {"nonzero": 1, "zero": 2}
LOGUP_MAX_FRACTIONS, LOGUP_MAX_COLUMNS = 4, 32


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
        if self.mask is None:
            mask = (0, 0)
        else:
            kind, m = self.mask
            if kind not in _MASK:
                raise ValueError(f"{who}: mask is None, ('nonzero', m) or ('zero', m), not {self.mask!r}")
            mask = (_MASK[kind], int(m))
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
