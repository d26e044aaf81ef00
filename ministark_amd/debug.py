"""`Stark::validate_constraints` (src/stark.rs:66-75) -- the check `default_prove` runs under debug_assertions (src/prover.rs:75)
and whose body, `default_validate_constraints` (src/debug.rs:10-127), is a stub in the reference.  Here it is implemented as its
commented-out intent describes: every constraint is evaluated at every row of the trace domain with the semantics of
`Constraint::check` (src/constraints.rs:172-248), on the device (ms_validate_constraints, csrc/validate_kernels.h).

Checked semantics, None written ⊥: Neg, Add and Pow (every exponent, 0 included) of ⊥ are ⊥; Mul of ⊥ and a defined zero is 0,
of ⊥ and anything else ⊥; Div(a, b) is lowered to Mul(a, Inv(b)) with Inv(⊥) = Inv(0) = ⊥.  That reproduces every arm of check's
Div but one: the reference gives Div(⊥, 0) = 0 (its arm reuses Mul's pattern), here it is ⊥ and the row is reported -- the
lowered program cannot tell that case from the others, and reporting is the conservative side.

A constraint fails at row i when its value at x_i = w_n^i is ⊥ (the trace domain is a subgroup; Trace(col, off) reads row
(i + off) mod n; Periodic leaves take the column's values on the trace domain, Goldilocks only)."""
import ctypes

import numpy as np

from . import expr as E
from .api import (GOLDILOCKS_FP, GOLDILOCKS_FQ3, STARK252_FP, GL_P, F252_P, Radix2EvaluationDomain, _ptr_array, f252_from_mont_limbs,
                  f252_to_mont_limbs, gl_from_mont, gl_to_mont)

NO_FAILURE = (1 << 64) - 1      # h_first_row of a constraint that holds on every row


class ConstraintViolation(AssertionError):
    """A constraint does not hold on the trace: the reference's panic in default_validate_constraints."""

    def __init__(self, message, constraint, row):
        super().__init__(message)
        self.constraint, self.row = constraint, row


class ValidationReport:
    """failures: (constraint index, first failing row, number of failing rows), in constraint order.  unused_columns / unused_challenges /
    unused_hints: the indices no constraint reads (the reference's "WARN: ..." lines)."""

    def __init__(self, failures, unused_columns, unused_challenges, unused_hints, message=None):
        self.failures = failures
        self.unused_columns, self.unused_challenges, self.unused_hints = unused_columns, unused_challenges, unused_hints
        self.message = message          # the report of the lowest failing constraint, or None

    @property
    def ok(self):
        return not self.failures

    def __repr__(self):
        return (f"ValidationReport(failures={self.failures}, unused_columns={self.unused_columns}, unused_challenges={self.unused_challenges}, "
                f"unused_hints={self.unused_hints})")


def compile_constraints(constraints, num_base_columns, fq_is_ext=True, base_field=GOLDILOCKS_FP):
    """ONE program for all the constraints: constraint k ends in STORE_P / STORE_Q with b = k.  Hash-consing runs across the
    constraints (a shared 1 / (X^n - 1) is computed once per row); no node is simplified away (Pow(⊥, 0) must stay ⊥)."""
    return E.lower(list(constraints), num_base_columns, fq_is_ext, base_field)


def _leaves(expr):
    """The leaves of one expression DAG, each node visited once (Expr::traverse)."""
    seen, stack, out = set(), [expr], []
    while stack:
        e = stack.pop()
        if id(e) in seen:
            continue
        seen.add(id(e))
        if e.kind in ("trace", "challenge", "hint"):
            out.append((e.kind,) + tuple(e.args))
        stack.extend(a for a in e.args if isinstance(a, E.Expr))
    return out


def _groups(constraints, nbase, fq_is_ext, base_field):
    """(first index, Program) per launch: all constraints in one program unless it needs more registers than the interpreter has."""
    out, todo = [], [(0, len(constraints))]
    while todo:
        lo, hi = todo.pop(0)
        try:
            out.append((lo, compile_constraints(constraints[lo:hi], nbase, fq_is_ext, base_field)))
        except ValueError as e:
            if "registers" not in str(e) or hi - lo == 1:
                raise
            mid = (lo + hi) // 2
            todo[:0] = [(lo, mid), (mid, hi)]
    return out


def _fmt(v):
    return f"CubicExtField({v[0]}, {v[1]}, {v[2]})" if isinstance(v, tuple) else str(v)


def _elem_words(v, fq_is_ext, base_field, what):
    if base_field == STARK252_FP:
        if isinstance(v, tuple):
            raise ValueError(f"{what}: the 252-bit field has no extension")
        return [int(w) for w in f252_to_mont_limbs(int(v) % F252_P)]
    if fq_is_ext:
        t = tuple(v) if isinstance(v, tuple) else (int(v), 0, 0)
        return [gl_to_mont(int(c) % GL_P) for c in t]
    if isinstance(v, tuple):
        raise ValueError(f"{what}: an Fq3 value for an Fq = Fp AIR")
    return [gl_to_mont(int(v) % GL_P)]


def _message(c, row, constraint, x, trace_value, challenges, hints):
    """The reference's report (src/debug.rs:97-121): the leaves' values, sorted and de-duplicated."""
    vals = {f"x = {x}"}
    for leaf in _leaves(constraint):
        if leaf[0] == "trace":
            vals.add(f"Trace(col={str(leaf[1]).rjust(3, '0')}, offset={str(leaf[2]).rjust(3, '0')}) = {_fmt(trace_value(leaf[1], leaf[2]))}")
        elif leaf[0] == "challenge":
            vals.add(f"Challenge({leaf[1]}) = {_fmt(challenges[leaf[1]])}")
        else:
            vals.add(f"Hint({leaf[1]}) = {_fmt(hints[leaf[1]])}")
    return (f"Constraint {c} does not evaluate to a low degree polynomial. Divide by zero occurs at row {row}.\n\n"
            "Expression values:\n" + "\n".join(sorted(vals)))


def validate_constraints(constraints, challenges, hints, base_trace, extension_trace=None, *, raise_on_failure=True, fq_is_ext=None):
    """Check a trace against its AIR on the device.  constraints: list of E.Expr (the AIR's constraints, in order); challenges / hints:
    canonical ints, or 3-tuples for Fq3 (as composer.py takes them); base_trace / extension_trace: Matrix of the trace's n rows (Fp / Fq3).
    fq_is_ext: whether Fq is the cubic extension (default: when there is an extension trace or an Fq3 challenge / hint).
    Returns a ValidationReport; raises ConstraintViolation for the lowest failing constraint when raise_on_failure is set."""
    constraints = list(constraints)
    challenges, hints = list(challenges), list(hints)
    pl, L = base_trace.planner, base_trace.planner.lib
    base_field = base_trace.field
    if base_field not in (GOLDILOCKS_FP, STARK252_FP):
        raise ValueError("the base trace must be over Goldilocks Fp or the 252-bit field")
    n, nbase = base_trace.num_rows(), base_trace.num_cols()
    if n < 2 or n & (n - 1):
        raise ValueError("the trace length must be a power of two >= 2")
    ext_cols = extension_trace.columns if extension_trace is not None else []
    if extension_trace is not None and (extension_trace.field != GOLDILOCKS_FQ3 or extension_trace.num_rows() != n):
        raise ValueError("the extension trace must be an Fq3 matrix of the base trace's length")
    if fq_is_ext is None:
        fq_is_ext = base_field == GOLDILOCKS_FP and (bool(ext_cols) or any(isinstance(v, tuple) for v in challenges + hints))
    for c in constraints:
        for leaf in _leaves(c):
            if leaf[0] == "trace" and leaf[1] >= nbase + len(ext_cols):
                raise ValueError(f"Trace({leaf[1]}, {leaf[2]}) names a column the trace does not have")
            if leaf[0] == "challenge" and leaf[1] >= len(challenges):
                raise ValueError(f"Challenge({leaf[1]}) is not among the {len(challenges)} challenges")
            if leaf[0] == "hint" and leaf[1] >= len(hints):
                raise ValueError(f"Hint({leaf[1]}) is not among the {len(hints)} hints")
    VP = ctypes.c_void_p
    first = np.full(len(constraints), NO_FAILURE, dtype=np.uint64)
    count = np.zeros(len(constraints), dtype=np.uint64)
    for lo, prog in (_groups(constraints, nbase, fq_is_ext, base_field) if constraints else []):
        consts = np.array(prog.consts, dtype=np.uint64)
        for table, vals, what in ((prog.challenge_slots, challenges, "challenge"), (prog.hint_slots, hints, "hint")):
            for idx, off in table.items():
                w = _elem_words(vals[idx], fq_is_ext, base_field, f"{what} {idx}")
                consts[off:off + len(w)] = w
        if prog.periodic and base_field != GOLDILOCKS_FP:
            raise ValueError("periodic columns are not implemented for the 252-bit field")
        per = [E.periodic_lde(pl, c, iv, 1, n, 1) for (c, iv) in prog.periodic]
        code = np.ascontiguousarray(np.array(prog.instrs, dtype=np.uint32).reshape(-1, 4))
        k = sum(1 for ins in prog.instrs if ins[0] in (E.OP_STORE_P, E.OP_STORE_Q))
        f = np.empty(k, dtype=np.uint64)
        cnt = np.empty(k, dtype=np.uint64)
        per_arr = (VP * max(1, len(per)))(*[p.ptr for p in per])
        per_len = (ctypes.c_uint * max(1, len(per)))(*[len(p) for p in per])
        L.check(L.ms_validate_constraints(pl.handle, base_field, code.ctypes.data, len(code), consts.ctypes.data if consts.size else None, consts.size,
                                          n.bit_length() - 1, _ptr_array(base_trace.columns), nbase, _ptr_array(ext_cols), len(ext_cols),
                                          per_arr, per_len, len(per), k, f.ctypes.data, cnt.ctypes.data))
        first[lo:lo + k], count[lo:lo + k] = f, cnt
    failures = [(c, int(first[c]), int(count[c])) for c in range(len(constraints)) if int(first[c]) != NO_FAILURE]
    used = {"trace": set(), "challenge": set(), "hint": set()}
    for c in constraints:
        for leaf in _leaves(c):
            used[leaf[0]].add(leaf[1])
    report = ValidationReport(failures, [i for i in range(nbase + len(ext_cols)) if i not in used["trace"]],
                              [i for i in range(len(challenges)) if i not in used["challenge"]], [i for i in range(len(hints)) if i not in used["hint"]])
    if failures:
        c, row, _ = failures[0]
        report.message = _failure_message(c, row, constraints[c], n, base_trace, extension_trace, challenges, hints)
        if raise_on_failure:
            raise ConstraintViolation(report.message, c, row)
    return report


def _failure_message(c, row, constraint, n, base_trace, extension_trace, challenges, hints):
    """The values of the failing row's leaves: ONE gather (ms_gather_rows) of the rows the constraint reads, per trace matrix."""
    base_field = base_trace.field
    nbase = base_trace.num_cols()
    offs = sorted({leaf[2] for leaf in _leaves(constraint) if leaf[0] == "trace"})
    rows = sorted({(row + o) % n for o in offs})
    where = {r: k for k, r in enumerate(rows)}
    got_b = base_trace.get_rows(rows) if rows else None
    got_e = extension_trace.get_rows(rows) if rows and extension_trace is not None else None
    bw = 4 if base_field == STARK252_FP else 1

    def trace_value(col, off):
        k = where[(row + off) % n]
        if col < nbase:
            w = got_b[k, bw * col:bw * col + bw]
            return f252_from_mont_limbs(w) if bw == 4 else gl_from_mont(int(w[0]))
        w = got_e[k, 3 * (col - nbase):3 * (col - nbase) + 3]
        return tuple(gl_from_mont(int(v)) for v in w)
    dom = Radix2EvaluationDomain(n, 1, base_field)
    x = pow(dom.group_gen, row, dom.p)
    return _message(c, row, constraint, x, trace_value, challenges, hints)
