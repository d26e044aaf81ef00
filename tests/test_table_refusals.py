"""Every refusal of twelve trace-table entry points -- ms_build_extension_columns, ms_build_logup_columns, ms_lookup_multiplicities,
ms_sort_rows, ms_permute_columns, ms_gap_plan, ms_gap_fill, ms_limb_decompose, ms_range_multiplicities, ms_bitwise_columns,
ms_bitwise_table, ms_bitwise_multiplicities -- replayed through the C ABI against tests/golden/table_refusals.json: the same return
code and the same ms_last_error text, word for word.  Each entry point's cases were recorded before it came to share its argument
checks with the others (ms_internal.h: BaseColumns, canon_named; ext_args.h; count_args.h), so the file pins what each one says and
WHICH refusal wins where two could fire.  Null arguments, counts and indices out of range, bad kinds and signs, the size limits, every overlap pair, and the checked
mode: a non-canonical element in a column the call names is refused, in one it does not name the call goes through (the two column
builders scan the whole base table and refuse both).

All buffers are slots of one small allocation (n = 8 rows; a size limit is refused before anything looks at a buffer), zero but for the
index and the elements that are >= p.  A case that is not refused is recorded with code 0 and no text.  "env" in a case: environment
variables set for the call (MS_RANGE_FORM, MS_BITWISE_FORM).

    python -m tests.test_table_refusals        records the file anew from the simulator build (only when a refusal is ADDED)"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import backends

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_refusals.json")
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FP, FQ3, F252 = 0, 1, 2
N, SLOT, NSLOTS = 8, 256, 40                     # a slot holds 8 rows of the widest field
ONES = 0xFFFFFFFFFFFFFFFF
NONE = -1


class S:
    """slot k of the arena (plus a byte offset): resolved to an address when the call is made"""

    def __init__(self, k, off=0):
        self.k, self.off = k, off


# the slots: base columns 0..3 (zero), 4: row 3 is not canonical over Fp, 5: row 3 is not canonical over Fp252
BASE = [S(0), S(1), S(2), S(3)]
BAD_FP, BAD_252 = S(4), S(5)
CHAL, BAD_CHAL = S(6), S(7)                      # two Fq3 challenges; component 1 of challenge 1 is not canonical
OUT = [S(8), S(9), S(10), S(11)]
PERM, START, REPORT = S(12), S(13), S(14)        # the identity index, n + 1 zero prefix sums, a report


class Env:
    def __init__(self, kind):
        self.pl = backends.planner(kind)
        self.L, self.h = self.pl.lib, self.pl.handle
        arena = np.zeros(NSLOTS * SLOT // 8, dtype=np.uint64)
        arena[BAD_FP.k * SLOT // 8 + 3] = ONES
        arena[BAD_252.k * SLOT // 8 + 12:BAD_252.k * SLOT // 8 + 16] = ONES
        arena[BAD_CHAL.k * SLOT // 8 + 4] = ONES
        arena[PERM.k * SLOT // 8:PERM.k * SLOT // 8 + N // 2].view(np.uint32)[:] = np.arange(N, dtype=np.uint32)
        p = ctypes.c_void_p()
        self.L.check(self.L.ms_alloc(self.h, arena.nbytes, ctypes.byref(p)))
        self.base = p.value
        self.L.check(self.L.ms_upload(self.h, self.base, arena.ctypes.data, arena.nbytes))
        self.keep = []

    def close(self):
        self.L.check(self.L.ms_ctx_set_checked(self.h, 0))
        self.L.check(self.L.ms_sync(self.h))
        self.L.check(self.L.ms_free(self.h, self.base))

    def addr(self, v):
        if isinstance(v, S):
            return self.base + v.k * SLOT + v.off
        return v                                 # None, or the context handle

    def table(self, v):
        """a list of slots (None: a null entry) -> a pointer table; None -> a null table"""
        if v is None:
            return None
        t = (ctypes.c_void_p * max(len(v), 1))(*[self.addr(x) for x in v])
        self.keep.append(t)
        return t

    def words(self, rows, dtype=np.int32):
        """records as rows of 32-bit words -> their address; None -> null"""
        if rows is None:
            return None
        a = np.array(rows, dtype=np.int64).astype(dtype).ravel()
        if a.size == 0:
            a = np.zeros(1, dtype=dtype)
        self.keep.append(a)
        return a.ctypes.data


def column(init=0, init_chal=0, mask=0, mask_col=0, inclusive=0, na=1, nb=1):
    return [init, init_chal, mask, mask_col, inclusive, na, nb, 0]


def term(col=0, off=0, chal=NONE, sign=1):
    return [col, off, chal, sign]


def call_ext(e, ctx=True, bf=FP, ef=FQ3, n=N, base=BASE, nbase=None, chal=CHAL, nchal=2, cols=(column(),), terms=(term(), term(1)), next=None, out=OUT):
    cols = None if cols is None else list(cols)
    return e.L.ms_build_extension_columns(e.h if ctx else None, bf, ef, n, e.table(base), len(base) if nbase is None else nbase, e.addr(chal), nchal,
                                          e.words(cols), e.words(None if terms is None else list(terms)), len(cols) if next is None else next, e.table(out))


def lcolumn(init=0, init_chal=0, mask=0, mask_col=0, inclusive=0, nf=1):
    return [init, init_chal, mask, mask_col, inclusive, nf, 0, 0]


def call_logup(e, ctx=True, bf=FP, ef=FQ3, n=N, base=BASE, nbase=None, chal=CHAL, nchal=2, cols=(lcolumn(),), fracs=((1, 1),), terms=(term(), term(1)),
               next=None, out=OUT):
    cols = None if cols is None else list(cols)
    return e.L.ms_build_logup_columns(e.h if ctx else None, bf, ef, n, e.table(base), len(base) if nbase is None else nbase, e.addr(chal), nchal,
                                      e.words(cols), e.words(None if fracs is None else list(fracs), np.uint32), e.words(None if terms is None else list(terms)),
                                      len(cols) if next is None else next, e.table(out))


def tup(cols=(0, 1), mask=0, mask_col=0):
    return list(cols) + [0] * (4 - len(cols)) + [mask, mask_col, 0, 0]


def call_lookup(e, ctx=True, field=FP, n=N, base=BASE, nbase=None, width=2, table=tup(), sets=(tup((1, 2)), tup((2, 1))), nsets=None, m=OUT[0], report=REPORT):
    sets = None if sets is None else list(sets)
    return e.L.ms_lookup_multiplicities(e.h if ctx else None, field, n, e.table(base), len(base) if nbase is None else nbase, width,
                                        e.words(None if table is None else [table]), e.words(sets), (len(sets) if sets else 0) if nsets is None else nsets,
                                        e.addr(m), e.addr(report))


def call_sort(e, ctx=True, field=FP, n=N, base=BASE, nbase=None, nkeys=2, key=tup(), perm=PERM, report=REPORT):
    return e.L.ms_sort_rows(e.h if ctx else None, field, n, e.table(base), len(base) if nbase is None else nbase, nkeys,
                            e.words(None if key is None else [key]), e.addr(perm), e.addr(report))


def call_permute(e, ctx=True, field=FP, n_src=N, src=BASE[:2], dst=OUT[:2], ncols=None, index=PERM, n_out=N):
    return e.L.ms_permute_columns(e.h if ctx else None, field, n_src, e.table(src), e.table(dst), len(src) if ncols is None else ncols, e.addr(index), n_out)


def spec(group=(0,), ngroup=None, counter=1, mask=0, mask_col=0):
    return list(group) + [0] * (3 - len(group)) + [len(group) if ngroup is None else ngroup, counter, mask, mask_col, 0]


def call_plan(e, ctx=True, field=FP, n_src=N, base=BASE, nbase=None, spec=spec(), perm=PERM, n=N, start=START, report=REPORT):
    return e.L.ms_gap_plan(e.h if ctx else None, field, n_src, e.table(base), len(base) if nbase is None else nbase, e.words(None if spec is None else [spec]),
                           e.addr(perm), n, e.addr(start), e.addr(report))


def call_fill(e, ctx=True, field=FP, n_src=N, base=BASE, nbase=None, perm=PERM, n=N, start=START, cols=((0, 0), (2, 1), (3, 0)), dst=OUT[:3], ncols=None,
              n_out=N):
    cols = None if cols is None else list(cols)
    return e.L.ms_gap_fill(e.h if ctx else None, field, n_src, e.table(base), len(base) if nbase is None else nbase, e.addr(perm), n, e.addr(start),
                           e.words(cols), e.table(dst), len(cols) if ncols is None else ncols, n_out)


def limb(src=0, dst0=2, nlimbs=2, bits=4, mask=0, mask_col=0):
    return [src, dst0, nlimbs, bits, mask, mask_col, 0, 0]


def call_limb(e, ctx=True, field=FP, n=N, base=BASE, nbase=None, specs=(limb(),), nspecs=None, report=REPORT):
    specs = None if specs is None else list(specs)
    return e.L.ms_limb_decompose(e.h if ctx else None, field, n, e.table(base), len(base) if nbase is None else nbase,
                                 e.words(specs), (len(specs) if specs else 0) if nspecs is None else nspecs, e.addr(report))


def rset(col=0, mask=0, mask_col=0):
    return [col, mask, mask_col, 0]


def call_range(e, ctx=True, field=FP, n=N, base=BASE, nbase=None, bits=3, sets=(rset(), rset(1)), nsets=None, n_m=N, m=OUT[0], report=REPORT):
    sets = None if sets is None else list(sets)
    return e.L.ms_range_multiplicities(e.h if ctx else None, field, n, e.table(base), len(base) if nbase is None else nbase, bits,
                                       e.words(sets), (len(sets) if sets else 0) if nsets is None else nsets, n_m, e.addr(m), e.addr(report))


AND, OR, XOR = 0, 1, 2


def bspec(op=AND, a=0, b=1, dst=2, width=8, mask=0, mask_col=0):
    return [op, a, b, dst, width, mask, mask_col, 0]


def call_bcols(e, ctx=True, field=FP, n=N, base=BASE, nbase=None, specs=(bspec(),), nspecs=None, report=REPORT):
    specs = None if specs is None else list(specs)
    return e.L.ms_bitwise_columns(e.h if ctx else None, field, n, e.table(base), len(base) if nbase is None else nbase,
                                  e.words(specs), (len(specs) if specs else 0) if nspecs is None else nspecs, e.addr(report))


# the table of 3 ops over pairs of 1-bit limbs has 12 rows: a column of it over Fp252 is a slot and a half
TOP, TX, TY, TZ = S(16), S(18), S(20), S(22)


def call_btable(e, ctx=True, field=FP, bits=1, ops=(AND, OR, XOR), nops=None, n_t=12, top=TOP, tx=TX, ty=TY, tz=TZ):
    return e.L.ms_bitwise_table(e.h if ctx else None, field, bits, e.words(None if ops is None else list(ops)), (len(ops) if ops else 0) if nops is None else nops,
                                n_t, e.addr(top), e.addr(tx), e.addr(ty), e.addr(tz))


def bset(op=AND, a=0, b=1, c=NONE, nlimbs=2, mask=0, mask_col=0):
    return [op, a, b, c, nlimbs, mask, mask_col, 0]


def call_bmult(e, ctx=True, field=FP, n=N, base=BASE, nbase=None, bits=1, ops=(AND, XOR), nops=None, sets=(bset(), bset(XOR, c=2)), nsets=None, n_m=N,
               m=OUT[0], report=REPORT):
    sets = None if sets is None else list(sets)
    return e.L.ms_bitwise_multiplicities(e.h if ctx else None, field, n, e.table(base), len(base) if nbase is None else nbase, bits,
                                         e.words(None if ops is None else list(ops)), (len(ops) if ops else 0) if nops is None else nops,
                                         e.words(sets), (len(sets) if sets else 0) if nsets is None else nsets, n_m, e.addr(m), e.addr(report))


BIG30, BIG32 = (1 << 30) + 1, (1 << 32) + 1
BASE_NULL2 = [S(0), S(1), None, S(3)]
WITH_BAD = [S(0), S(1), BAD_FP, S(3)]            # column 2 is the one that is not canonical
WITH_BAD_252 = [S(0), S(1), BAD_252, S(3)]

# (case, arguments that differ from the call's defaults); "checked": the context's checked mode is on for the call
ENTRIES = {
    "ms_build_extension_columns": (call_ext, [
        ("accepted", {}),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null d_challenges", dict(chal=None)),
        ("null h_columns", dict(cols=None, next=1)),
        ("null d_out", dict(out=None)),
        ("null h_terms", dict(terms=None)),
        ("base field fq3", dict(bf=FQ3)),
        ("fp to fp252", dict(ef=F252)),
        ("fp252 to fq3", dict(bf=F252)),
        ("unknown field", dict(bf=9)),
        ("33 columns", dict(cols=[column(na=0, nb=0)] * 33, terms=None, out=OUT * 9)),
        ("9 a terms", dict(cols=[column(na=9)])),
        ("9 b terms", dict(cols=[column(nb=9)])),
        ("null base column", dict(base=BASE_NULL2)),
        ("null output column", dict(cols=[column(), column()], terms=[term()] * 4, out=[OUT[0], None])),
        ("init kind -1", dict(cols=[column(init=-1)])),
        ("init kind 3", dict(cols=[column(init=3)])),
        ("init challenge -1", dict(cols=[column(init=2, init_chal=-1)])),
        ("init challenge 2", dict(cols=[column(init=2, init_chal=2)])),
        ("init challenge without challenges", dict(cols=[column(init=2)], chal=None, nchal=0)),
        ("mask kind -1", dict(cols=[column(mask=-1)])),
        ("mask kind 3", dict(cols=[column(mask=3)])),
        ("mask column -1", dict(cols=[column(mask=1, mask_col=-1)])),
        ("mask column 4", dict(cols=[column(mask=2, mask_col=4)])),
        ("mask column ignored when always", dict(cols=[column(mask=0, mask_col=99)])),
        ("term column -2", dict(terms=[term(-2), term()])),
        ("term column 4", dict(terms=[term(), term(4)])),
        ("term challenge -2", dict(terms=[term(chal=-2), term()])),
        ("term challenge 2", dict(terms=[term(), term(chal=2)])),
        ("sign 0", dict(terms=[term(sign=0), term()])),
        ("sign 2", dict(terms=[term(), term(sign=2)])),
        ("second column names the column", dict(cols=[column(), column(mask=3)], terms=[term()] * 4)),
        ("init before mask", dict(cols=[column(init=7, mask=7)])),
        ("mask before term", dict(cols=[column(mask=7)], terms=[term(9), term()])),
        ("term column before term challenge before sign", dict(terms=[term(9, chal=9, sign=0), term()])),
        ("term challenge before sign", dict(terms=[term(chal=9, sign=0), term()])),
        ("null output before init", dict(cols=[column(init=7)], out=[None])),
        ("null base column before null output", dict(base=BASE_NULL2, out=[None])),
        ("column too long", dict(n=1 << 42)),
        ("n 0 passes the overlap", dict(n=0, out=[S(0)])),
        ("output and base overlap", dict(out=[S(1, 8)])),
        ("output and unnamed base overlap", dict(out=[S(3)])),
        ("outputs overlap", dict(cols=[column(), column()], terms=[term()] * 4, out=[OUT[0], S(OUT[0].k, 64)])),
        ("output and challenges overlap", dict(out=[S(CHAL.k, 40)])),
        ("the first output's refusal first", dict(cols=[column(), column()], terms=[term()] * 4, out=[CHAL, S(0)])),
        ("checked: named column", dict(checked=True, base=WITH_BAD, terms=[term(2), term()])),
        ("checked: unnamed column", dict(checked=True, base=WITH_BAD)),
        ("checked: fp252", dict(checked=True, bf=F252, ef=F252, base=WITH_BAD_252, nchal=1)),
        ("checked: challenges", dict(checked=True, chal=BAD_CHAL)),
        ("checked: canonical", dict(checked=True)),
        ("checked: overlap first", dict(checked=True, base=WITH_BAD, out=[S(1)])),
    ]),
    "ms_build_logup_columns": (call_logup, [
        ("accepted", {}),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null d_challenges", dict(chal=None)),
        ("null h_columns", dict(cols=None, next=1)),
        ("null d_out", dict(out=None)),
        ("null h_fractions", dict(fracs=None)),
        ("null h_terms", dict(terms=None)),
        ("base field fq3", dict(bf=FQ3)),
        ("fp252 to fq3", dict(bf=F252)),
        ("unknown field", dict(ef=9)),
        ("33 columns", dict(cols=[lcolumn(nf=0)] * 33, fracs=None, terms=None, out=OUT * 9)),
        ("5 fractions", dict(cols=[lcolumn(nf=5)])),
        ("9 numerator terms", dict(fracs=[(9, 1)])),
        ("9 denominator terms", dict(fracs=[(0, 9)])),
        ("null base column", dict(base=BASE_NULL2)),
        ("null output column", dict(out=[None])),
        ("init kind 3", dict(cols=[lcolumn(init=3)])),
        ("init challenge 2", dict(cols=[lcolumn(init=2, init_chal=2)])),
        ("init challenge -1", dict(cols=[lcolumn(init=2, init_chal=-1)])),
        ("mask kind 3", dict(cols=[lcolumn(mask=3)])),
        ("mask kind -1", dict(cols=[lcolumn(mask=-1)])),
        ("mask column 4", dict(cols=[lcolumn(mask=1, mask_col=4)])),
        ("mask column -1", dict(cols=[lcolumn(mask=2, mask_col=-1)])),
        ("no denominator", dict(fracs=[(1, 0)], terms=[term()])),
        ("no denominator in the second fraction", dict(cols=[lcolumn(nf=2)], fracs=[(1, 1), (2, 0)], terms=[term()] * 4)),
        ("term column 4", dict(terms=[term(), term(4)])),
        ("term column -2", dict(terms=[term(-2), term()])),
        ("term challenge 2", dict(terms=[term(chal=2), term()])),
        ("term challenge -2", dict(terms=[term(), term(chal=-2)])),
        ("sign 0", dict(terms=[term(), term(sign=0)])),
        ("sign -2", dict(terms=[term(sign=-2), term()])),
        ("second column names the column", dict(cols=[lcolumn(), lcolumn(init=5)], fracs=[(1, 1), (1, 1)], terms=[term()] * 4)),
        ("init before mask", dict(cols=[lcolumn(init=7, mask=7)])),
        ("mask before denominator", dict(cols=[lcolumn(mask=7)], fracs=[(1, 0)])),
        ("denominator before term", dict(fracs=[(1, 0)], terms=[term(9)])),
        ("term column before term challenge before sign", dict(terms=[term(9, chal=9, sign=0), term()])),
        ("fraction count before null base column", dict(base=BASE_NULL2, fracs=[(9, 1)])),
        ("column too long", dict(n=1 << 42)),
        ("next 0 passes", dict(cols=[], fracs=None, terms=None, out=[])),
        ("output and base overlap", dict(out=[S(2, 8)])),
        ("outputs overlap", dict(cols=[lcolumn(), lcolumn()], fracs=[(1, 1), (1, 1)], terms=[term()] * 4, out=[OUT[1], S(OUT[1].k, 8)])),
        ("output and challenges overlap", dict(out=[CHAL])),
        ("checked: named column", dict(checked=True, base=WITH_BAD, terms=[term(2), term()])),
        ("checked: unnamed column", dict(checked=True, base=WITH_BAD)),
        ("checked: challenges", dict(checked=True, chal=BAD_CHAL)),
        ("checked: canonical", dict(checked=True)),
    ]),
    "ms_lookup_multiplicities": (call_lookup, [
        ("accepted", {}),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_table", dict(table=None)),
        ("null h_lookups", dict(sets=None, nsets=1)),
        ("no sets", dict(sets=None)),
        ("null d_m", dict(m=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=7)),
        ("width 0", dict(width=0)),
        ("width 5", dict(width=5)),
        ("9 sets", dict(sets=[tup()] * 9)),
        ("null base column", dict(base=BASE_NULL2)),
        ("table column 4", dict(table=tup((0, 4)))),
        ("table column -1", dict(table=tup((-1, 0)))),
        ("set column 4", dict(sets=[tup(), tup((4, 0))])),
        ("column past the width is not read", dict(table=[0, 1, 99, 99, 0, 0, 0, 0])),
        ("table mask kind 3", dict(table=tup(mask=3))),
        ("set mask kind -1", dict(sets=[tup(mask=-1)])),
        ("table mask column 4", dict(table=tup(mask=1, mask_col=4))),
        ("set mask column -1", dict(sets=[tup(), tup(mask=2, mask_col=-1)])),
        ("column before mask", dict(table=tup((0, 9), mask=9))),
        ("table before sets", dict(table=tup(mask=9), sets=[tup((9, 9))])),
        ("width before sets before null base column", dict(base=BASE_NULL2, width=9, sets=[tup()] * 9)),
        ("rows 2^30 + 1", dict(n=BIG30)),
        ("8 sets of 2^29 rows", dict(n=1 << 29, sets=[tup()] * 8)),
        ("column before rows", dict(n=BIG30, table=tup((0, 4)))),
        ("d_m and named base overlap", dict(m=S(1, 8))),
        ("d_m and the mask's column overlap", dict(table=tup(mask=1, mask_col=3), m=S(3))),
        ("d_m is an unnamed base column", dict(m=S(3))),
        ("d_report and named base overlap", dict(report=S(2, 56))),
        ("d_m and d_report overlap", dict(report=S(OUT[0].k, 8))),
        ("base before d_m and d_report", dict(m=S(0), report=S(0))),
        ("n 0", dict(n=0)),
        ("checked: named column", dict(checked=True, base=WITH_BAD)),
        ("checked: the mask's column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP], table=tup(mask=1, mask_col=3))),
        ("checked: unnamed column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP])),
        ("checked: fp252", dict(checked=True, field=F252, base=WITH_BAD_252)),
        ("checked: n 0", dict(checked=True, n=0, base=WITH_BAD)),
    ]),
    "ms_sort_rows": (call_sort, [
        ("accepted", {}),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_key", dict(key=None)),
        ("null d_perm", dict(perm=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=-3)),
        ("0 keys", dict(nkeys=0)),
        ("5 keys", dict(nkeys=5)),
        ("null base column", dict(base=BASE_NULL2)),
        ("key column 4", dict(key=tup((0, 4)))),
        ("key column -1", dict(key=tup((-1, 0)))),
        ("column past the keys is not read", dict(key=[0, 1, 99, 99, 0, 0, 0, 0])),
        ("mask kind 3", dict(key=tup(mask=3))),
        ("mask kind -1", dict(key=tup(mask=-1))),
        ("mask column 4", dict(key=tup(mask=1, mask_col=4))),
        ("mask column -1", dict(key=tup(mask=2, mask_col=-1))),
        ("key column before mask", dict(key=tup((9, 0), mask=9))),
        ("keys before null base column", dict(base=BASE_NULL2, nkeys=0)),
        ("rows 2^30 + 1", dict(n=BIG30)),
        ("mask before rows", dict(n=BIG30, key=tup(mask=1, mask_col=9))),
        ("d_perm and named base overlap", dict(perm=S(0, 28))),
        ("d_perm and the mask's column overlap", dict(key=tup(mask=2, mask_col=3), perm=S(3))),
        ("d_perm in an unnamed base column", dict(perm=S(3))),
        ("d_report and named base overlap", dict(report=S(1, 56))),
        ("d_perm and d_report overlap", dict(report=S(PERM.k, 24))),
        ("d_perm before d_report", dict(perm=S(0), report=S(0))),
        ("n 0", dict(n=0)),
        ("checked: named column", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: the mask's column", dict(checked=True, base=WITH_BAD, key=tup(mask=1, mask_col=2))),
        ("checked: unnamed column", dict(checked=True, base=WITH_BAD)),
        ("checked: fp252", dict(checked=True, field=F252, base=[BAD_252, S(1), S(2), S(3)])),
        ("checked: n 0", dict(checked=True, n=0, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
    "ms_permute_columns": (call_permute, [
        ("accepted", {}),
        ("accepted over fq3", dict(field=FQ3)),
        ("null ctx", dict(ctx=False)),
        ("null d_src", dict(src=None, ncols=2)),
        ("null d_dst", dict(dst=None)),
        ("null d_index", dict(index=None)),
        ("unknown field", dict(field=3)),
        ("0 columns", dict(ncols=0)),
        ("129 columns", dict(src=BASE[:2] * 65, dst=OUT[:2] * 65, ncols=129)),
        ("null source column", dict(src=[S(0), None])),
        ("null destination column", dict(dst=[None, OUT[1]])),
        ("source rows 2^32 + 1", dict(n_src=BIG32)),
        ("destination and source overlap", dict(dst=[OUT[0], S(0, 56)])),
        ("destination and another source overlap", dict(dst=[S(1), OUT[1]])),
        ("destination and index overlap", dict(dst=[OUT[0], S(PERM.k, 24)])),
        ("destinations overlap", dict(dst=[OUT[0], S(OUT[0].k, 56)])),
        ("the first destination's refusal first", dict(dst=[PERM, S(0)])),
        ("source before index", dict(dst=[OUT[0], S(0)], index=S(0, 8))),
        ("n_out 0", dict(n_out=0)),
        ("n_out 0 still checks", dict(n_out=0, ncols=0)),
    ]),
    "ms_gap_plan": (call_plan, [
        ("accepted", {}),
        ("accepted without an index", dict(perm=None)),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_spec", dict(spec=None)),
        ("null d_start", dict(start=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=11)),
        ("null base column", dict(base=BASE_NULL2)),
        ("group of -1", dict(spec=spec(ngroup=-1))),
        ("group of 4", dict(spec=spec(ngroup=4))),
        ("group column 4", dict(spec=spec((0, 4)))),
        ("group column -1", dict(spec=spec((-1,)))),
        ("counter column 4", dict(spec=spec(counter=4))),
        ("no counter", dict(spec=spec(counter=-1))),
        ("counter -2 is no counter", dict(spec=spec(counter=-2))),
        ("mask kind 3", dict(spec=spec(mask=3))),
        ("mask kind -1", dict(spec=spec(mask=-1))),
        ("mask column 4", dict(spec=spec(mask=1, mask_col=4))),
        ("mask column -1", dict(spec=spec(mask=2, mask_col=-1))),
        ("null base column before group", dict(base=BASE_NULL2, spec=spec(ngroup=4))),
        ("group before counter before mask", dict(spec=spec((9,), counter=9, mask=9))),
        ("counter before mask", dict(spec=spec(counter=9, mask=9))),
        ("positions 2^30 + 1", dict(n=BIG30)),
        ("source rows 2^32 + 1", dict(n_src=BIG32)),
        ("positions before source rows", dict(n=BIG30, n_src=BIG32)),
        ("mask before positions", dict(n=BIG30, spec=spec(mask=1, mask_col=9))),
        ("d_start and named base overlap", dict(start=S(0, 56))),
        ("d_start and the mask's column overlap", dict(spec=spec(mask=1, mask_col=3), start=S(3))),
        ("d_start in an unnamed base column", dict(start=S(3))),
        ("d_report and named base overlap", dict(report=S(1))),
        ("d_start and d_perm overlap", dict(start=S(PERM.k, 24))),
        ("d_report and d_perm overlap", dict(report=S(PERM.k, 24))),
        ("d_start and d_report overlap", dict(report=S(START.k, 64))),
        ("base before d_perm", dict(start=S(0), perm=S(0))),
        ("n 0", dict(n=0)),
        ("checked: the group's column", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)])),
        ("checked: the counter's column", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: the mask's column", dict(checked=True, base=WITH_BAD, spec=spec(mask=2, mask_col=2))),
        ("checked: unnamed column", dict(checked=True, base=WITH_BAD)),
        ("checked: fp252", dict(checked=True, field=F252, base=[S(0), BAD_252, S(2), S(3)])),
        ("checked: n 0", dict(checked=True, n=0, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
    "ms_gap_fill": (call_fill, [
        ("accepted", {}),
        ("accepted without an index", dict(perm=None)),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null d_start", dict(start=None)),
        ("null h_columns", dict(cols=None, ncols=1)),
        ("null d_dst", dict(dst=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=5)),
        ("0 columns", dict(ncols=0)),
        ("129 columns", dict(cols=[(0, 0)] * 129, dst=OUT * 33)),
        ("null base column", dict(base=BASE_NULL2)),
        ("null destination", dict(dst=[OUT[0], None, OUT[2]])),
        ("kind 4", dict(cols=[(0, 0), (4, 0), (0, 0)])),
        ("kind -1", dict(cols=[(-1, 0), (0, 0), (0, 0)])),
        ("source column 4", dict(cols=[(0, 0), (1, 4), (0, 0)])),
        ("source column -1", dict(cols=[(2, -1), (0, 0), (0, 0)])),
        ("a flag names no source", dict(cols=[(3, 99), (0, 0), (0, 0)])),
        ("null destination before kind before source", dict(cols=[(9, 9), (0, 0), (0, 0)], dst=[None, OUT[1], OUT[2]])),
        ("kind before source", dict(cols=[(9, 9), (0, 0), (0, 0)])),
        ("columns before null base column", dict(base=BASE_NULL2, ncols=0)),
        ("positions 2^30 + 1", dict(n=BIG30)),
        ("output rows 2^30 + 1", dict(n_out=BIG30)),
        ("source rows 2^32 + 1", dict(n_src=BIG32)),
        ("positions before output rows before source rows", dict(n=BIG30, n_out=BIG30, n_src=BIG32)),
        ("destination and named base overlap", dict(dst=[OUT[0], S(1, 56), OUT[2]])),
        ("destination in an unnamed base column", dict(dst=[OUT[0], OUT[1], S(3)])),
        ("a flag's destination and named base overlap", dict(dst=[OUT[0], OUT[1], S(0)])),
        ("destination and d_perm overlap", dict(dst=[S(PERM.k, 24), OUT[1], OUT[2]])),
        ("destination and d_start overlap", dict(dst=[OUT[0], S(START.k, 64), OUT[2]])),
        ("destinations overlap", dict(dst=[OUT[0], OUT[1], S(OUT[0].k, 56)])),
        ("the first destination's refusal comes first", dict(dst=[PERM, START, S(0)])),
        ("n_out 0", dict(n_out=0)),
        ("checked: named column", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: unnamed column", dict(checked=True, base=WITH_BAD)),
        ("checked: only flags name nothing", dict(checked=True, base=[BAD_FP, BAD_FP, S(2), S(3)], cols=[(3, 0)], dst=OUT[:1])),
        ("checked: fp252", dict(checked=True, field=F252, base=[BAD_252, S(1), S(2), S(3)])),
        ("checked: n_out 0", dict(checked=True, n_out=0, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
    "ms_limb_decompose": (call_limb, [
        ("accepted", {}),
        ("accepted over fp252", dict(field=F252)),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_specs", dict(specs=None, nspecs=1)),
        ("no specs", dict(specs=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=7)),
        ("65 specs", dict(specs=[limb()] * 65)),
        ("rows 2^32 + 1", dict(n=BIG32)),
        ("rows 2^32 are not refused for their number", dict(n=1 << 32, specs=[limb(src=9)])),
        ("null base column", dict(base=BASE_NULL2)),
        ("source column 4", dict(specs=[limb(src=4)])),
        ("source column -1", dict(specs=[limb(), limb(src=-1, dst0=1, nlimbs=1)])),
        ("mask kind 3", dict(specs=[limb(mask=3)])),
        ("mask kind -1", dict(specs=[limb(mask=-1)])),
        ("mask column 4", dict(specs=[limb(mask=1, mask_col=4)])),
        ("mask column -1", dict(specs=[limb(mask=2, mask_col=-1)])),
        ("mask column ignored when always", dict(specs=[limb(mask=0, mask_col=99)])),
        ("0 bits", dict(specs=[limb(bits=0)])),
        ("33 bits", dict(specs=[limb(bits=33)])),
        ("0 limbs", dict(specs=[limb(nlimbs=0)])),
        ("257 limbs", dict(specs=[limb(nlimbs=257)])),
        ("5 limbs of 16 bits over fp", dict(specs=[limb(nlimbs=5, bits=16)])),
        ("9 limbs of 32 bits over fp252", dict(field=F252, specs=[limb(nlimbs=9, bits=32)])),
        ("2 limbs of 32 bits over fp", dict(specs=[limb(nlimbs=2, bits=32)])),
        ("destination -1", dict(specs=[limb(dst0=-1)])),
        ("destination 4", dict(specs=[limb(dst0=4)])),
        ("destinations past the table", dict(specs=[limb(dst0=3, nlimbs=2)])),
        ("source before mask before bits before limbs before destination", dict(specs=[limb(src=9, mask=9, bits=0, nlimbs=0, dst0=9)])),
        ("mask before bits before limbs before destination", dict(specs=[limb(mask=9, bits=0, nlimbs=0, dst0=9)])),
        ("bits before limbs before destination", dict(specs=[limb(bits=0, nlimbs=0, dst0=9)])),
        ("limbs before their width before destination", dict(specs=[limb(bits=32, nlimbs=300, dst0=9)])),
        ("width before destination", dict(specs=[limb(bits=32, nlimbs=3, dst0=9)])),
        ("rows before specs", dict(n=BIG32, specs=[limb(src=9)])),
        ("count before null base column", dict(base=BASE_NULL2, specs=[limb()] * 65)),
        ("destinations of two specs overlap", dict(specs=[limb(0, 2, 2), limb(1, 3, 1)])),
        ("destinations of the first and third spec overlap", dict(specs=[limb(0, 1, 1, mask=0), limb(0, 2, 1), limb(0, 1, 3)])),
        ("two destination columns in the same memory go through", dict(base=[S(0), S(1), S(2), S(2)])),
        ("two specs' destinations in the same memory go through", dict(base=[S(0), S(1), S(2), S(2, 8)], specs=[limb(0, 2, 1), limb(1, 3, 1)])),
        ("destination is the source", dict(specs=[limb(0, 0, 1)])),
        ("destination is another spec's source", dict(specs=[limb(0, 2, 1), limb(2, 3, 1)])),
        ("destination is a later spec's mask", dict(specs=[limb(0, 2, 2), limb(0, 1, 1, mask=1, mask_col=3)])),
        ("destination and source memory overlap", dict(base=[S(0), S(1), S(0, 56), S(3)], specs=[limb(0, 2, 1)])),
        ("second destination and mask memory overlap", dict(base=[S(0), S(1), S(2), S(1, 8)], specs=[limb(0, 2, 2, mask=1, mask_col=1)])),
        ("destination and unnamed column memory overlap goes through", dict(base=[S(0), S(2), S(2), S(3)], specs=[limb(0, 2, 1)])),
        ("d_report and source overlap", dict(report=S(0, 56))),
        ("d_report and the mask's column overlap", dict(specs=[limb(mask=2, mask_col=1)], report=S(1))),
        ("d_report and destination overlap", dict(report=S(3, 8))),
        ("d_report in an unnamed column", dict(report=S(1))),
        ("the first spec's source before the second's destinations", dict(specs=[limb(0, 0, 1), limb(1, 0, 1)])),
        ("two specs' destinations before the second's source", dict(specs=[limb(0, 2, 1), limb(2, 2, 1)])),
        ("destinations before d_report", dict(specs=[limb(0, 2, 1), limb(1, 2, 1)], report=S(0))),
        ("a read column before a destination for d_report", dict(base=[S(0), S(1), S(2), S(2, 64)], specs=[limb(3, 2, 1)], report=S(2, 56))),
        ("a later spec's destinations before d_report and the first's destination", dict(specs=[limb(0, 2, 1), limb(1, 2, 1)], report=S(2))),
        ("n 0", dict(n=0)),
        ("n 0 passes the memory overlaps", dict(n=0, base=[S(0), S(1), S(0), S(3)], report=S(0))),
        ("n 0 still refuses a destination that is the source", dict(n=0, specs=[limb(0, 0, 1)])),
        ("checked: source", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)])),
        ("checked: the mask's column", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)], specs=[limb(mask=1, mask_col=1)])),
        ("checked: unnamed column", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: destination", dict(checked=True, base=WITH_BAD)),
        ("checked: fp252", dict(checked=True, field=F252, base=[BAD_252, S(1), S(2), S(3)])),
        ("checked: overlap first", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)], report=S(2))),
        ("checked: n 0", dict(checked=True, n=0, base=[BAD_FP, S(1), S(2), S(3)])),
        ("checked: no specs", dict(checked=True, specs=None, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
    "ms_range_multiplicities": (call_range, [
        ("accepted", {}),
        ("accepted over fp252", dict(field=F252)),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_sets", dict(sets=None, nsets=1)),
        ("no sets", dict(sets=None)),
        ("null d_m", dict(m=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=7)),
        ("0 bits", dict(bits=0)),
        ("25 bits", dict(bits=25)),
        ("65 sets", dict(sets=[rset()] * 65)),
        ("d_m of 7", dict(n_m=7)),
        ("d_m of 2^24 - 1 for 24 bits", dict(bits=24, n_m=(1 << 24) - 1)),
        ("null base column", dict(base=BASE_NULL2)),
        ("set column 4", dict(sets=[rset(), rset(4)])),
        ("set column -1", dict(sets=[rset(-1)])),
        ("mask kind 3", dict(sets=[rset(mask=3)])),
        ("mask kind -1", dict(sets=[rset(), rset(mask=-1)])),
        ("mask column 4", dict(sets=[rset(mask=1, mask_col=4)])),
        ("mask column -1", dict(sets=[rset(mask=2, mask_col=-1)])),
        ("column before mask", dict(sets=[rset(9, mask=9)])),
        ("bits before sets before d_m before null base column", dict(base=BASE_NULL2, bits=0, sets=[rset()] * 65, n_m=0)),
        ("sets before d_m before null base column", dict(base=BASE_NULL2, sets=[rset()] * 65, n_m=0)),
        ("d_m before null base column", dict(base=BASE_NULL2, n_m=0)),
        ("rows 2^32 + 1", dict(n=BIG32)),
        ("2 sets of 2^31 rows", dict(n=1 << 31)),
        ("1 set of 2^32 rows", dict(n=1 << 32, sets=[rset()])),
        ("column before rows", dict(n=BIG32, sets=[rset(4)])),
        ("rows before counters", dict(n=BIG32, sets=[rset()] * 64)),
        ("d_m and named base overlap", dict(m=S(1, 8))),
        ("d_m and the mask's column overlap", dict(sets=[rset(mask=1, mask_col=3)], m=S(3))),
        ("d_m is an unnamed base column", dict(m=S(3))),
        ("d_report and named base overlap", dict(report=S(1, 56))),
        ("d_report in an unnamed base column", dict(report=S(2))),
        ("d_m and d_report overlap", dict(report=S(OUT[0].k, 56))),
        ("d_m before d_report on one column", dict(m=S(0), report=S(0))),
        ("the first column's d_report before the second's d_m", dict(m=S(1), report=S(0))),
        ("base before d_m and d_report", dict(m=S(1), report=S(1, 8))),
        ("bad MS_RANGE_FORM", dict(env={"MS_RANGE_FORM": "fast"})),
        ("empty MS_RANGE_FORM", dict(env={"MS_RANGE_FORM": ""})),
        ("MS_RANGE_FORM plain", dict(env={"MS_RANGE_FORM": "plain"})),
        ("MS_RANGE_FORM lds", dict(env={"MS_RANGE_FORM": "lds"})),
        ("overlap before MS_RANGE_FORM", dict(env={"MS_RANGE_FORM": "fast"}, m=S(0))),
        ("n 0", dict(n=0)),
        ("n 0 reads MS_RANGE_FORM", dict(n=0, env={"MS_RANGE_FORM": "fast"})),
        ("checked: named column", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: the mask's column", dict(checked=True, base=WITH_BAD, sets=[rset(mask=1, mask_col=2)])),
        ("checked: unnamed column", dict(checked=True, base=WITH_BAD)),
        ("checked: d_m is an unnamed column", dict(checked=True, base=WITH_BAD, m=BAD_FP)),
        ("checked: fp252", dict(checked=True, field=F252, base=[BAD_252, S(1), S(2), S(3)])),
        ("checked: before MS_RANGE_FORM", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)], env={"MS_RANGE_FORM": "fast"})),
        ("checked: n 0", dict(checked=True, n=0, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
    "ms_bitwise_columns": (call_bcols, [
        ("accepted", {}),
        ("accepted with one operand twice", dict(specs=[bspec(XOR, 1, 1)])),
        ("accepted over fp252", dict(field=F252, specs=[bspec(OR, width=251)])),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_specs", dict(specs=None, nspecs=1)),
        ("no specs", dict(specs=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=7)),
        ("65 specs", dict(specs=[bspec()] * 65)),
        ("rows 2^32 + 1", dict(n=BIG32)),
        ("rows 2^32 are not refused for their number", dict(n=1 << 32, specs=[bspec(op=9)])),
        ("null base column", dict(base=BASE_NULL2)),
        ("op 3", dict(specs=[bspec(op=3)])),
        ("op -1", dict(specs=[bspec(), bspec(op=-1, dst=3)])),
        ("operand a 4", dict(specs=[bspec(a=4)])),
        ("operand a -1", dict(specs=[bspec(a=-1)])),
        ("operand b 4", dict(specs=[bspec(b=4)])),
        ("operand b -1", dict(specs=[bspec(b=-1)])),
        ("mask kind 3", dict(specs=[bspec(mask=3)])),
        ("mask kind -1", dict(specs=[bspec(mask=-1)])),
        ("mask column 4", dict(specs=[bspec(mask=1, mask_col=4)])),
        ("mask column -1", dict(specs=[bspec(mask=2, mask_col=-1)])),
        ("width 0", dict(specs=[bspec(width=0)])),
        ("width 63 over fp", dict(specs=[bspec(width=63)])),
        ("width 64 over fp", dict(specs=[bspec(width=64)])),
        ("width 252 over fp252", dict(field=F252, specs=[bspec(width=252)])),
        ("destination -1", dict(specs=[bspec(dst=-1)])),
        ("destination 4", dict(specs=[bspec(dst=4)])),
        ("op before a before b before mask before width before destination", dict(specs=[bspec(op=9, a=9, b=9, mask=9, width=0, dst=9)])),
        ("a before b before mask before width before destination", dict(specs=[bspec(a=9, b=9, mask=9, width=0, dst=9)])),
        ("b before mask before width before destination", dict(specs=[bspec(b=9, mask=9, width=0, dst=9)])),
        ("mask before width before destination", dict(specs=[bspec(mask=9, width=0, dst=9)])),
        ("width before destination", dict(specs=[bspec(width=0, dst=9)])),
        ("rows before specs", dict(n=BIG32, specs=[bspec(op=9)])),
        ("count before null base column", dict(base=BASE_NULL2, specs=[bspec()] * 65)),
        ("two specs with one destination", dict(specs=[bspec(), bspec(OR)])),
        ("the first and third spec with one destination", dict(specs=[bspec(dst=3), bspec(dst=2), bspec(XOR, dst=3)])),
        ("two specs' destinations in the same memory", dict(base=[S(0), S(1), S(2), S(2, 56)], specs=[bspec(dst=2), bspec(dst=3)])),
        ("destination is operand a", dict(specs=[bspec(a=2)])),
        ("destination is operand b", dict(specs=[bspec(b=2)])),
        ("destination is another spec's operand", dict(specs=[bspec(dst=2), bspec(a=2, dst=3)])),
        ("destination is a later spec's mask", dict(specs=[bspec(dst=2), bspec(dst=3, mask=1, mask_col=2)])),
        ("destination and operand memory overlap", dict(base=[S(0), S(1), S(1, 56), S(3)])),
        ("destination and mask memory overlap", dict(base=[S(0), S(1), S(2), S(2, 8)], specs=[bspec(mask=2, mask_col=3)])),
        ("destination and unnamed column memory overlap goes through", dict(base=[S(0), S(1), S(2), S(2)])),
        ("d_report and operand overlap", dict(report=S(1, 56))),
        ("d_report and the mask's column overlap", dict(specs=[bspec(mask=2, mask_col=3)], report=S(3))),
        ("d_report and destination overlap", dict(report=S(2, 8))),
        ("d_report in an unnamed column", dict(report=S(3))),
        ("the first spec's operand before the second's destination", dict(specs=[bspec(a=2), bspec(dst=2)])),
        ("two specs' destinations before the second's operand", dict(specs=[bspec(dst=2), bspec(a=2, dst=2)])),
        ("a destination before a read column for d_report", dict(base=[S(0), S(1), S(2), S(2, 64)], specs=[bspec(a=3)], report=S(2, 56))),
        ("d_report and the first's destination before a later spec's destination", dict(specs=[bspec(), bspec(OR)], report=S(2))),
        ("the first spec's operand before d_report and its destination", dict(specs=[bspec(a=2)], report=S(2))),
        ("n 0", dict(n=0)),
        ("n 0 passes the memory overlaps", dict(n=0, base=[S(0), S(1), S(0), S(3)], report=S(0))),
        ("n 0 still refuses a destination that is an operand", dict(n=0, specs=[bspec(b=2)])),
        ("checked: operand a", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)])),
        ("checked: operand b", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: the mask's column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP], specs=[bspec(mask=1, mask_col=3)])),
        ("checked: unnamed column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP])),
        ("checked: destination", dict(checked=True, base=WITH_BAD)),
        ("checked: fp252", dict(checked=True, field=F252, base=[S(0), BAD_252, S(2), S(3)])),
        ("checked: overlap first", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)], report=S(2))),
        ("checked: n 0", dict(checked=True, n=0, base=[BAD_FP, S(1), S(2), S(3)])),
        ("checked: no specs", dict(checked=True, specs=None, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
    "ms_bitwise_table": (call_btable, [
        ("accepted", {}),
        ("accepted without an op column", dict(top=None)),
        ("accepted over fp252", dict(field=F252)),
        ("accepted with one op", dict(ops=[XOR], n_t=4)),
        ("null ctx", dict(ctx=False)),
        ("null h_ops", dict(ops=None, nops=3)),
        ("null d_tx", dict(tx=None)),
        ("null d_ty", dict(ty=None)),
        ("null d_tz", dict(tz=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=7)),
        ("0 bits", dict(bits=0)),
        ("13 bits", dict(bits=13)),
        ("0 ops", dict(ops=[AND], nops=0)),
        ("4 ops", dict(ops=[AND, OR, XOR, AND])),
        ("op 3", dict(ops=[AND, 3])),
        ("op -1", dict(ops=[-1])),
        ("op named twice", dict(ops=[OR, XOR, OR])),
        ("unknown op before an op named twice", dict(ops=[5, OR, OR])),
        ("an op named twice before an unknown one", dict(ops=[OR, OR, 5])),
        ("2 ops over 12 bits", dict(bits=12, ops=[AND, OR], n_t=1 << 25)),
        ("1 op over 12 bits is 2^24 rows, too few elements", dict(bits=12, ops=[AND], n_t=(1 << 24) - 1)),
        ("11 elements", dict(n_t=11)),
        ("bits before ops before elements", dict(bits=0, ops=[9], n_t=0)),
        ("ops before elements", dict(ops=[9], n_t=0)),
        ("d_tx and d_ty overlap", dict(ty=S(TX.k, 88))),
        ("d_tx and d_tz overlap", dict(tz=S(TX.k, 88))),
        ("d_ty and d_tz overlap", dict(tz=S(TY.k, 88))),
        ("d_tx and d_top overlap", dict(top=S(TX.k, 88))),
        ("d_ty and d_top overlap", dict(top=S(TY.k, 88))),
        ("d_tz and d_top overlap", dict(top=S(TZ.k, 88))),
        ("columns that touch do not overlap", dict(ty=S(TX.k, 96))),
        ("d_tx and d_ty before d_tx and d_tz", dict(ty=TX, tz=TX)),
        ("d_ty and d_tz before d_tx and d_top", dict(tz=TY, top=TX)),
        ("elements before overlap", dict(n_t=11, ty=TX)),
    ]),
    "ms_bitwise_multiplicities": (call_bmult, [
        ("accepted", {}),
        ("accepted over fp252", dict(field=F252)),
        ("null ctx", dict(ctx=False)),
        ("null d_base", dict(base=None, nbase=4)),
        ("null h_ops", dict(ops=None, nops=2)),
        ("null h_sets", dict(sets=None, nsets=1)),
        ("no sets", dict(sets=None)),
        ("null d_m", dict(m=None)),
        ("null d_report", dict(report=None)),
        ("fq3", dict(field=FQ3)),
        ("unknown field", dict(field=7)),
        ("0 bits", dict(bits=0)),
        ("13 bits", dict(bits=13)),
        ("0 ops", dict(ops=[AND], nops=0)),
        ("4 ops", dict(ops=[AND, OR, XOR, AND])),
        ("table op 3", dict(ops=[AND, 3])),
        ("table op named twice", dict(ops=[XOR, XOR])),
        ("2 ops over 12 bits", dict(bits=12, ops=[AND, OR], n_m=1 << 25)),
        ("65 sets", dict(sets=[bset()] * 65)),
        ("d_m of 7", dict(n_m=7)),
        ("null base column", dict(base=BASE_NULL2)),
        ("set op 5", dict(sets=[bset(op=5)])),
        ("set op not in the table", dict(sets=[bset(), bset(OR)])),
        ("operand a 4", dict(sets=[bset(a=4)])),
        ("operand a -1", dict(sets=[bset(a=-1)])),
        ("operand b 4", dict(sets=[bset(b=4)])),
        ("operand b -1", dict(sets=[bset(b=-1)])),
        ("result -2", dict(sets=[bset(c=-2)])),
        ("result 4", dict(sets=[bset(c=4)])),
        ("mask kind 3", dict(sets=[bset(mask=3)])),
        ("mask kind -1", dict(sets=[bset(mask=-1)])),
        ("mask column 4", dict(sets=[bset(mask=1, mask_col=4)])),
        ("mask column -1", dict(sets=[bset(mask=2, mask_col=-1)])),
        ("0 limbs", dict(sets=[bset(nlimbs=0)])),
        ("257 limbs", dict(sets=[bset(nlimbs=257)])),
        ("63 limbs of 1 bit over fp", dict(sets=[bset(nlimbs=63)])),
        ("64 limbs of 1 bit over fp", dict(sets=[bset(nlimbs=64)])),
        ("252 limbs of 1 bit over fp252", dict(field=F252, sets=[bset(nlimbs=252)])),
        ("6 limbs of 12 bits over fp", dict(bits=12, ops=[AND], n_m=1 << 24, sets=[bset(nlimbs=6)])),
        ("bits before ops before sets before d_m before null base column", dict(base=BASE_NULL2, bits=0, ops=[9], sets=[bset()] * 65, n_m=0)),
        ("ops before sets before d_m before null base column", dict(base=BASE_NULL2, ops=[9], sets=[bset()] * 65, n_m=0)),
        ("sets before d_m before null base column", dict(base=BASE_NULL2, sets=[bset()] * 65, n_m=0)),
        ("d_m before null base column", dict(base=BASE_NULL2, n_m=0)),
        ("unknown op before an op not in the table before a before b before result before mask before limbs",
         dict(sets=[bset(op=5, a=9, b=9, c=9, mask=9, nlimbs=0)])),
        ("an op not in the table before a before b before result before mask before limbs", dict(sets=[bset(op=OR, a=9, b=9, c=9, mask=9, nlimbs=0)])),
        ("a before b before result before mask before limbs", dict(sets=[bset(a=9, b=9, c=9, mask=9, nlimbs=0)])),
        ("b before result before mask before limbs", dict(sets=[bset(b=9, c=-9, mask=9, nlimbs=0)])),
        ("result before mask before limbs", dict(sets=[bset(c=-9, mask=9, nlimbs=0)])),
        ("mask before limbs", dict(sets=[bset(mask=9, nlimbs=0)])),
        ("limbs before their width", dict(sets=[bset(nlimbs=300)])),
        ("rows 2^32 + 1", dict(n=BIG32)),
        ("2 limbs a row over 2^31 rows", dict(n=1 << 31, sets=[bset()])),
        ("1 limb a row over 2^32 rows", dict(n=1 << 32, sets=[bset(nlimbs=1)])),
        ("set before rows", dict(n=BIG32, sets=[bset(a=4)])),
        ("rows before counters", dict(n=BIG32, sets=[bset()] * 64)),
        ("d_m and operand a overlap", dict(m=S(0, 56))),
        ("d_m and operand b overlap", dict(m=S(1, 8))),
        ("d_m and the result column overlap", dict(m=S(2))),
        ("d_m and the mask's column overlap", dict(sets=[bset(mask=1, mask_col=3)], m=S(3))),
        ("d_m is an unnamed base column", dict(m=S(3))),
        ("d_report and named base overlap", dict(report=S(2, 56))),
        ("d_report in an unnamed base column", dict(report=S(3))),
        ("d_m and d_report overlap", dict(report=S(OUT[0].k, 56))),
        ("d_m before d_report on one column", dict(m=S(0), report=S(0))),
        ("the first column's d_report before the second's d_m", dict(m=S(1), report=S(0))),
        ("base before d_m and d_report", dict(m=S(1), report=S(1, 8))),
        ("bad MS_BITWISE_FORM", dict(env={"MS_BITWISE_FORM": "fast"})),
        ("empty MS_BITWISE_FORM", dict(env={"MS_BITWISE_FORM": ""})),
        ("MS_BITWISE_FORM plain", dict(env={"MS_BITWISE_FORM": "plain"})),
        ("MS_BITWISE_FORM lds", dict(env={"MS_BITWISE_FORM": "lds"})),
        ("overlap before MS_BITWISE_FORM", dict(env={"MS_BITWISE_FORM": "fast"}, m=S(0))),
        ("n 0", dict(n=0)),
        ("n 0 reads MS_BITWISE_FORM", dict(n=0, env={"MS_BITWISE_FORM": "fast"})),
        ("checked: operand a", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)])),
        ("checked: operand b", dict(checked=True, base=[S(0), BAD_FP, S(2), S(3)])),
        ("checked: the result column", dict(checked=True, base=WITH_BAD)),
        ("checked: the mask's column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP], sets=[bset(mask=1, mask_col=3)])),
        ("checked: unnamed column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP])),
        ("checked: d_m is an unnamed column", dict(checked=True, base=[S(0), S(1), S(2), BAD_FP], m=BAD_FP)),
        ("checked: fp252", dict(checked=True, field=F252, base=[BAD_252, S(1), S(2), S(3)])),
        ("checked: before MS_BITWISE_FORM", dict(checked=True, base=[BAD_FP, S(1), S(2), S(3)], env={"MS_BITWISE_FORM": "fast"})),
        ("checked: n 0", dict(checked=True, n=0, base=[BAD_FP, S(1), S(2), S(3)])),
    ]),
}


def replay(kind, entry):
    """-> [(entry, case, code, text)] of every case of the entry point, in order, each on a fresh arena"""
    fn, cases = ENTRIES[entry]
    out = []
    for case, args in cases:
        env = Env(kind)
        args = dict(args)
        setenv = args.pop("env", {})
        try:
            env.L.check(env.L.ms_ctx_set_checked(env.h, 1 if args.pop("checked", False) else 0))
            os.environ.update(setenv)
            rc = fn(env, **args)
            out.append([entry, case, rc, env.L.ms_last_error().decode() if rc else None])
        finally:
            for name in setenv:
                del os.environ[name]
            env.close()
    return out


@pytest.fixture(scope="module")
def golden():
    return [tuple(r) for r in json.load(open(GOLDEN))]


def test_the_golden_file_lists_the_cases(golden):
    assert [(e, c) for e, c, _, _ in golden] == [(e, c) for e, (_, cases) in ENTRIES.items() for c, _ in cases]
    assert len({(e, c) for e, c, _, _ in golden}) == len(golden)
    refused = [r for r in golden if r[2]]
    assert all(r[2] in (-1, -2) and r[3].startswith(r[0] + ": ") or r[3].startswith("unknown field id") for r in refused)
    assert all(r[3] is None for r in golden if not r[2])
    # in the checked mode a column the call does not name goes through everywhere but in the two column builders, which scan the table
    for e, c, code, _ in golden:
        if c == "checked: unnamed column":
            assert (code == 0) == (e not in ("ms_build_extension_columns", "ms_build_logup_columns")), e


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_refusal_is_the_recorded_one(kind, entry, golden):
    want = [r for r in golden if r[0] == entry]
    got = [tuple(r) for r in replay(kind, entry)]
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff and len(got) == len(want), "\n".join(f"{g}\n   recorded: {w}" for g, w in diff)


if __name__ == "__main__":
    rows = [r for entry in ENTRIES for r in replay("emu", entry)]
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} cases -> {GOLDEN}")
