"""validate_constraints (ministark_amd/debug.py, ms_validate_constraints, csrc/validate_kernels.h) against a checked reference model
written here: Constraint::check's semantics (src/constraints.rs:172-248) over the E.Expr DAG -- not over the lowered program -- with
oracle.pyref.fields for the arithmetic, and the documented deviation Div(⊥, 0) = ⊥ (the reference's arm gives 0)."""
import ast
import os

import numpy as np
import pytest

from tests import backends
from tests.test_verifier_relations import fib_trace
from oracle.pyref.fields import F252, FQ3, GL
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ, STARK252_FP, Matrix, pipeline
from ministark_amd import expr as E
from ministark_amd.api import Radix2EvaluationDomain, _ptr_array, f252_to_mont_limbs, gl_to_mont
from ministark_amd.debug import ConstraintViolation, NO_FAILURE, compile_constraints, validate_constraints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = pytest.param("emu", id="emu")
HIP = pytest.param("hip", id="hip", marks=pytest.mark.gpu)
BACKENDS = [EMU, HIP]


# ---- the checked reference model ---------------------------------------------------------------------------------------------------
def model(constraints, n, base, ext, challenges, hints, fq_is_ext, field=GL, rows=None):
    """[(first failing row, rows failed)] per constraint over `rows` (default: all n).  base / ext: lists of canonical values per column
    (ints / 3-tuples); challenges / hints canonical.  None is ⊥."""
    F = field
    w = F.root_of_unity(n)
    rows = range(n) if rows is None else rows
    res = [[NO_FAILURE, 0] for _ in constraints]
    isq = lambda v: isinstance(v, tuple)
    lift = lambda v: v if isq(v) else (v, 0, 0)
    zero = lambda v: v == (0, 0, 0) if isq(v) else v == 0
    nb = len(base)

    def fq(v):
        return (lift(v) if fq_is_ext else v)

    for r in rows:
        x = F.pow(w, r)
        memo = {}

        def ev(e):
            if id(e) in memo:
                return memo[id(e)]
            k, a = e.kind, e.args
            if k == "x":
                v = x
            elif k == "const":
                v = (a[1] % F.p) if a[0] == E.FP else tuple(c % GL.p for c in a[1])
            elif k == "challenge":
                v = fq(challenges[a[0]])
            elif k == "hint":
                v = fq(hints[a[0]])
            elif k == "trace":
                col, off = a
                j = (r + off) % n
                v = base[col][j] if col < nb else ext[col - nb][j]
            elif k == "periodic":
                coeffs, iv = a
                y = F.pow(x, n // iv)
                v = 0
                for c in reversed(coeffs):
                    v = F.add(F.mul(v, y), c)
            elif k == "neg":
                s = ev(a[0])
                v = None if s is None else (FQ3.neg(s) if isq(s) else F.neg(s))
            elif k == "pow":
                s = ev(a[0])
                v = None if s is None else (FQ3.pow(s, a[1]) if isq(s) else F.pow(s, a[1]))
            else:
                p, q = ev(a[0]), ev(a[1])
                if k == "div":                      # Mul(p, Inv(q)): Inv(⊥) = Inv(0) = ⊥
                    q = None if q is None or zero(q) else (FQ3.inv(q) if isq(q) else F.inv(q))
                ext_ = (p is not None and isq(p)) or (q is not None and isq(q))
                if ext_:
                    p = None if p is None else lift(p)
                    q = None if q is None else lift(q)
                if k == "add":
                    v = None if p is None or q is None else (FQ3.add(p, q) if ext_ else F.add(p, q))
                elif p is not None and q is not None:
                    v = FQ3.mul(p, q) if ext_ else F.mul(p, q)
                elif p is None and q is None:
                    v = None
                else:
                    d = p if q is None else q
                    v = d if zero(d) else None      # Mul(⊥, 0) = 0
            memo[id(e)] = v
            return v
        for c, con in enumerate(constraints):
            if ev(con) is None:
                res[c][0] = min(res[c][0], r)
                res[c][1] += 1
    return [tuple(t) for t in res]


def failures_of(m):
    return [(c, f, k) for c, (f, k) in enumerate(m) if k]


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def gl_mont(cols):
    return [np.array([gl_to_mont(v) for v in c], dtype=np.uint64) for c in cols]


def gl_matrix(pl, cols):
    return Matrix.from_numpy(pl, gl_mont(cols), FP)


def fq_matrix(pl, cols):
    return Matrix.from_numpy(pl, [np.array([gl_to_mont(x) for v in c for x in v], dtype=np.uint64) for c in cols], FQ)


def f252_matrix(pl, cols):
    return Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(v) for v in c]) for c in cols], STARK252_FP)


_FIB = {}


def fib_cols(n):
    if n not in _FIB:
        _FIB[n] = fib_trace(n)
    return [list(c) for c in _FIB[n]]


def fib_trace252(n):
    """gen_trace of examples/fib over the 252-bit field."""
    p = F252.p
    cols = [[0] * n for _ in range(8)]
    v = [1, 2]
    for k in range(2, 8):
        v.append(v[k - 2] * v[k - 1] % p)
    for r in range(n):
        for k in range(8):
            cols[k][r] = v[k]
        w = [v[6] * v[7] % p]
        w.append(v[7] * w[0] % p)
        for k in range(2, 8):
            w.append(w[k - 2] * w[k - 1] % p)
        v = w
    return cols


# ---- 1. fib AIR, valid trace --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log_n", [pytest.param("emu", 10, id="emu-2^10"), pytest.param("hip", 10, id="hip-2^10", marks=pytest.mark.gpu),
                                        pytest.param("hip", 20, id="hip-2^20", marks=pytest.mark.gpu)])
def test_fib_air_valid_trace(kind, log_n):
    pl = backends.planner(kind)
    n = 1 << log_n
    cols = fib_cols(n)
    cons = pipeline.fib_air_constraints(n)
    hints = [cols[7][n - 1], 12345]                   # the claimed n-th value + one hint no constraint reads
    r = validate_constraints(cons, [99], hints, gl_matrix(pl, cols))
    assert r.ok and r.failures == [] and r.message is None
    assert (r.unused_columns, r.unused_challenges, r.unused_hints) == ([], [0], [1])
    if log_n <= 10:
        assert failures_of(model(cons, n, cols, [], [99], hints, False)) == []


# ---- 2. fib AIR, corrupted cells ----------------------------------------------------------------------------------------------------
def _corruptions(n):
    # (column, row): row 0, an interior row, row n - 1, and a cell only a `next` offset reads (column 2 is read at offset 0 only by its
    # boundary constraint, which is defined away from row 0)
    return [(7, 0), (6, n // 2 + 1), (7, n - 1), (2, n // 2 + 9)]


@pytest.mark.parametrize("kind", BACKENDS)
def test_fib_air_corrupted_cells(kind):
    pl = backends.planner(kind)
    n = 1 << 8
    cons = pipeline.fib_air_constraints(n)
    for col, row in _corruptions(n):
        cols = fib_cols(n)
        cols[col][row] = (cols[col][row] + 1) % GL.p
        hints = [fib_cols(n)[7][n - 1]]
        want = failures_of(model(cons, n, cols, [], [], hints, False))
        assert want, (col, row)
        r = validate_constraints(cons, [], hints, gl_matrix(pl, cols), raise_on_failure=False)
        assert r.failures == want, (col, row)
        with pytest.raises(ConstraintViolation) as ei:
            validate_constraints(cons, [], hints, gl_matrix(pl, cols))
        c, first, _ = want[0]
        assert ei.value.constraint == c and ei.value.row == first
        msg = str(ei.value)
        assert msg.startswith(f"Constraint {c} does not evaluate to a low degree polynomial. Divide by zero occurs at row {first}.\n\nExpression values:\n")
        lines = msg.split("Expression values:\n")[1].split("\n")
        assert lines == sorted(set(lines))
        x = pow(Radix2EvaluationDomain(n, 1, FP).group_gen, first, GL.p)
        assert f"x = {x}" in lines
        if c < 8:                                      # a boundary constraint reads Trace(c, 0) at the failing row
            assert f"Trace(col=00{c}, offset=000) = {cols[c][first]}" in lines


@pytest.mark.gpu
def test_fib_air_corrupted_cells_2_20():
    pl = backends.planner("hip")
    n = 1 << 20
    cons = pipeline.fib_air_constraints(n)
    cols = fib_cols(n)
    good = gl_mont(cols)
    hints = [cols[7][n - 1]]
    for col, row in _corruptions(n):
        was = cols[col][row]
        cols[col][row] = (was + 1) % GL.p
        mont = [c.copy() for c in good]
        mont[col][row] = gl_to_mont(cols[col][row])
        window = sorted({(row + d) % n for d in range(-2, 3)} | {0, n - 1})      # the rows that read the cell (offsets 0, 1), and the boundaries
        want = failures_of(model(cons, n, cols, [], [], hints, False, rows=window))
        cols[col][row] = was
        r = validate_constraints(cons, [], hints, Matrix.from_numpy(pl, mont, FP), raise_on_failure=False)
        assert r.failures == want, (col, row)         # equal counts: every row outside the window passes


# ---- 3. wrong hint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BACKENDS)
def test_wrong_hint_fails_only_the_terminal_constraint(kind):
    pl = backends.planner(kind)
    n = 1 << 8
    cols = fib_cols(n)
    cons = pipeline.fib_air_constraints(n)
    hints = [(cols[7][n - 1] + 5) % GL.p]
    r = validate_constraints(cons, [], hints, gl_matrix(pl, cols), raise_on_failure=False)
    assert r.failures == [(8, n - 1, 1)]
    assert r.failures == failures_of(model(cons, n, cols, [], [], hints, False))
    assert f"Hint(0) = {hints[0]}" in r.message.split("\n")


# ---- 4. extension AIR (running product over Fq3) ------------------------------------------------------------------------------------
def _ext_air(n):
    x = E.X()
    last = pow(Radix2EvaluationDomain(n, 1, FP).group_gen, n - 1, GL.p)
    b, e = E.Trace(0, 0), (lambda o=0: E.Trace(1, o))
    zer = (x - E.Constant(last)) / (x ** n - E.Constant(1))
    return [(e(1) - e() * (E.Challenge(0) - b * E.Challenge(1))) * zer, (e() - E.Constant(1)) / (x - E.Constant(1))]


def _ext_trace(n, g0, g1, seed=5):
    rng = np.random.default_rng(seed)
    b = [int(v) for v in rng.integers(0, 1 << 62, size=n)]
    e = [(1, 0, 0)]
    for i in range(n - 1):
        e.append(FQ3.mul(e[-1], FQ3.sub(g0, FQ3.mul_base(g1, b[i]))))
    return b, e


@pytest.mark.parametrize("kind", BACKENDS)
def test_extension_air(kind):
    pl = backends.planner(kind)
    n = 1 << 8
    g = [(11, 22, 33), (44, 55, 66)]
    cons = _ext_air(n)
    b, e = _ext_trace(n, *g)
    prog = compile_constraints(cons, 1, True)
    assert any(ins[0] == E.OP_STORE_Q for ins in prog.instrs)
    r = validate_constraints(cons, g, [], gl_matrix(pl, [b]), fq_matrix(pl, [e]))
    assert r.failures == [] and r.unused_columns == [] and r.unused_challenges == []
    for row in (0, 77, n - 1):
        bad = list(e)
        bad[row] = (bad[row][0], (bad[row][1] + 1) % GL.p, bad[row][2])      # one component only
        want = failures_of(model(cons, n, [b], [bad], g, [], True))
        assert want
        r = validate_constraints(cons, g, [], gl_matrix(pl, [b]), fq_matrix(pl, [bad]), raise_on_failure=False)
        assert r.failures == want, row
        if want[0][0] == 0:
            k = want[0][1]
            assert f"Trace(col=001, offset=001) = CubicExtField{bad[(k + 1) % n]}" in r.message.split("\n")


# ---- 5. the 252-bit field -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BACKENDS)
def test_fib_air_over_the_252_bit_field(kind):
    pl = backends.planner(kind)
    n = 1 << 6
    cols = fib_trace252(n)
    cons = pipeline.fib_air_constraints(n, STARK252_FP)
    hints = [cols[7][n - 1]]
    r = validate_constraints(cons, [], hints, f252_matrix(pl, cols))
    assert r.failures == []
    cols[3][n // 2] = (cols[3][n // 2] + 1) % F252.p
    want = failures_of(model(cons, n, cols, [], [], hints, False, field=F252))
    assert want
    r = validate_constraints(cons, [], hints, f252_matrix(pl, cols), raise_on_failure=False)
    assert r.failures == want


# ---- 6. the semantics, one rule per constraint ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BACKENDS)
def test_checked_semantics(kind):
    pl = backends.planner(kind)
    n = 1 << 5
    a, z = E.Trace(0), E.Trace(1)                       # a = row mod 3, z = 0
    nonzero_a = [(r, ) for r in range(n) if r % 3]
    cases = [
        (z / z, []),                                    # 0 / 0 = Mul(0, ⊥) = 0
        (a / z, nonzero_a),                             # a / 0
        (z * (a / z), []),                              # 0 * ⊥ = 0
        ((a / z) + z, nonzero_a),                       # ⊥ + 0
        ((a / z) ** 0, nonzero_a),                      # ⊥^0 = ⊥, not 1
        (-(a / z), nonzero_a),
        (E.Constant((1, 0, 0)) / E.Constant((0, 0, 0)), [(r, ) for r in range(n)]),    # Fq3 zero: all three components
        (E.Constant((1, 0, 0)) / E.Constant((0, 1, 0)), []),
        ((a / z) / z, nonzero_a),                       # Div(⊥, 0): ⊥ here, 0 in the reference (documented deviation)
    ]
    cons = [c for c, _ in cases]
    cols = [[r % 3 for r in range(n)], [0] * n]
    want = [(k, rows[0][0], len(rows)) for k, (_, rows) in enumerate(cases) if rows]
    assert failures_of(model(cons, n, cols, [], [], [], True)) == want
    r = validate_constraints(cons, [], [], gl_matrix(pl, cols), raise_on_failure=False, fq_is_ext=True)
    assert r.failures == want


# ---- 7. fuzz: tests/fuzz_eval.py's random DAGs ----------------------------------------------------------------------------------------
def _rand_expr_factory(rng):
    """tests/fuzz_eval.py's rand_expr, taken from the file as it is (the script runs its fuzz loop when imported)."""
    src = open(os.path.join(ROOT, "tests", "fuzz_eval.py")).read()
    fn = next(node for node in ast.parse(src).body if isinstance(node, ast.FunctionDef) and node.name == "rand_expr")
    ns = {"rng": rng, "E": E, "BOUNDARY": []}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "tests/fuzz_eval.py", "exec"), ns)
    return ns


@pytest.mark.parametrize("kind", BACKENDS)
def test_fuzz_against_the_model(kind):
    pl = backends.planner(kind)
    rng = np.random.default_rng(2024)
    ns = _rand_expr_factory(rng)
    cases = int(os.environ.get("MS_VALIDATE_FUZZ_CASES", "300"))
    for case in range(cases):
        log_n = int(rng.choice([3, 4, 5]))
        n = 1 << log_n
        fq_is_ext = bool(rng.integers(0, 2))
        nbase, next_, nch = int(rng.integers(1, 4)), (int(rng.integers(0, 3)) if fq_is_ext else 0), int(rng.integers(0, 3))
        dom = Radix2EvaluationDomain(n, 1, FP)
        ns["BOUNDARY"][:] = [pow(dom.group_gen, int(r) % n, dom.p) for r in rng.integers(-20, 21, size=4)]
        cons = [ns["rand_expr"](int(rng.integers(2, 6)), nbase, next_, nch, log_n) for _ in range(int(rng.integers(1, 4)))]
        small = lambda k: [int(v) for v in rng.integers(0, 3, size=k)]
        base = [small(n) for _ in range(nbase)]
        ext = [[tuple(small(3)) for _ in range(n)] for _ in range(next_)]
        ch = [tuple(small(3)) if fq_is_ext else small(1)[0] for _ in range(max(nch, 1))]
        want = failures_of(model(cons, n, base, ext, ch, [], fq_is_ext))
        r = validate_constraints(cons, ch, [], gl_matrix(pl, base), fq_matrix(pl, ext) if ext else None, raise_on_failure=False,
                                 fq_is_ext=fq_is_ext)
        assert r.failures == want, f"case {case}: log_n={log_n} fq_is_ext={fq_is_ext}"


# ---- 8. periodic leaf; error paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BACKENDS)
def test_periodic_leaf(kind):
    pl = backends.planner(kind)
    n = 1 << 6
    per = E.Periodic([0, 1, 0, 0], 4)                   # the column's polynomial is y: values w_4^(i mod 4), never zero
    t = E.Trace(0)
    cons = [t / (per - E.Constant(1)), (t - per) / (t - per)]
    cols = [[pow(GL.root_of_unity(4), r % 4, GL.p) if r % 5 else 0 for r in range(n)]]
    want = failures_of(model(cons, n, cols, [], [], [], False))
    assert want and want[0][0] == 0                     # rows 4k with t != 0 fail the first constraint
    r = validate_constraints(cons, [], [], gl_matrix(pl, cols), raise_on_failure=False)
    assert r.failures == want


@pytest.mark.parametrize("kind", BACKENDS)
def test_error_paths(kind):
    pl = backends.planner(kind)
    L = pl.lib
    n = 1 << 4
    col = gl_matrix(pl, [[1] * n])
    cols = _ptr_array(col.columns)
    f = np.empty(4, dtype=np.uint64)
    c = np.empty(4, dtype=np.uint64)

    def call(prog, nconstraints, field=FP, base=cols, nbase=1):
        code = np.ascontiguousarray(np.array(prog, dtype=np.uint32).reshape(-1, 4))
        consts = np.zeros(8, dtype=np.uint64)
        return L.ms_validate_constraints(pl.handle, field, code.ctypes.data, len(code), consts.ctypes.data, 8, 4, base, nbase, None, 0,
                                         None, None, 0, nconstraints, f.ctypes.data, c.ctypes.data)
    ok = [(E.OP_TRACE_P, 0, 0, 0), (E.OP_STORE_P, 0, 0, 0)]
    assert call(ok, 1) == 0 and f[0] == NO_FAILURE and c[0] == 0
    assert call([(E.OP_TRACE_P, 0, 0, 0), (E.OP_STORE_P, 0, 0, 1)], 1) == -1                        # store index >= nconstraints
    assert call([(E.OP_TRACE_P, 0, 0, 0), (E.OP_STORE_P, 0, 0, 0), (E.OP_STORE_P, 0, 0, 0)], 2) == -1  # index stored twice
    assert call([(E.OP_CONST_Q, 0, 0, 0), (E.OP_STORE_Q, 0, 0, 0)], 1, field=STARK252_FP) == -1     # a Q op with the 252-bit field
    assert call(ok, 1, base=None) == -1                                                            # null column table
    assert call(ok, 0) == -1                                                                       # no constraints
    assert call([(22, 0, 0, 0), (E.OP_STORE_P, 0, 0, 0)], 1) == -1                                 # an internal opcode
    assert call(ok, 1, field=FQ) == -1                                                             # not a base field
    assert "ms_validate_constraints" in L.ms_last_error().decode()
    with pytest.raises(ValueError):
        validate_constraints([E.Trace(3)], [], [], col)                                            # a column the trace lacks
