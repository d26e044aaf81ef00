"""The data-parallel phases of `default_prove` (src/prover.rs:25-174) for an Fq = Fp AIR, device-resident,
sequenced over the mirror in api.py / expr.py / composer.py -- what BASELINE.json's "end-to-end prove time"
measures on this backend (configs[4], the C5 shape: fib-like trace, ProofOptions::new(32, 4, 8, 8, 64),
examples/fib/main.rs:225).

The Fiat-Shamir channel (src/channel.rs: SHA-256 over a few digests, host work in the reference too) is
replaced by draws the caller fixes in advance, so that the CPU oracle can follow the same transcript and every
intermediate commitment can be compared (tests/test_pipeline_parity.py):
    interpolate + LDE + commit            prover.rs:50-55
    constraint evaluation                 prover.rs:88-107   (on the committed bit-reversed layout)
    composition trace                     prover.rs:111-124  (iNTT, split into ce_blowup columns, LDE, commit)
    DEEP composition + its LDE            prover.rs:137-152  (composer.rs:43-188)
    FRI layers: commit + fold             fri.rs:179-231
    FRI remainder                         fri.rs:232-248     (bit_reverse, iNTT on the subgroup; the first n / blowup coefficients)
    proof of work                         prover.rs:160, channel.rs:76-93
    trace / composition query openings    prover.rs:163-173  (trace.rs:113-157)
    FRI layer openings                    prover.rs:161, fri.rs:148-165, 615-622 (fold_positions, rows + Merkle views per layer)
What differs from a real run, on purpose: (i) the draws are fixed, so the proof-of-work seed is the last FRI root instead
of the channel's running digest (the same SHA-256 search either way); (ii) traces are random columns, not valid executions
(the data-parallel work does not depend on validity), so fri.rs:244's assertion that the remainder's high coefficients
vanish is not made; (iii) the composition constraint is lowered to its register program once per expression object, not once per proof
(an AIR's constraints are fixed; `_lowered`).  Proof serialisation and the channel's hashing of a few digests stay on the host in the reference too.
`prove` (below) runs the same phases with the channel in place: every challenge comes from a device-resident public coin (coin.py).
"""
import time

import numpy as np

from . import expr as E
from .api import (F252_P, GL_P, GOLDILOCKS_FP, STARK252_FP, Matrix, MerkleTree, Queries, Radix2EvaluationDomain, apply_drp, f252_to_mont_limbs,
                  gl_to_mont, grind_proof_of_work, pow_hash)
from .composer import DeepCompositionCoeffs, DeepPolyComposer


def _degree(e, trace_degree):
    """`Constraint::degree` (src/constraints.rs:32-41, 152-158, 407-455): an upper bound (numerator, denominator) on the
    degree in X, with the reference's own (loose) arithmetic."""
    k, a = e.kind, e.args
    if k in ("const", "challenge", "hint"):
        return (0, 0)
    if k == "trace":
        return (trace_degree, 0)
    if k == "x":
        return (1, 0)
    if k == "periodic":                                   # PeriodicColumn::degree (src/constraints.rs:135-141)
        coeffs, interval = a[0], a[1]
        return ((len(coeffs) - 1) * ((trace_degree + 1) // interval), 0)
    if k == "neg":
        return _degree(a[0], trace_degree)
    if k == "pow":
        n, d = _degree(a[0], trace_degree)
        return (n * a[1], d * a[1])
    (an, ad), (bn, bd) = _degree(a[0], trace_degree), _degree(a[1], trace_degree)
    if k == "add":
        return (max(an + bd, bn + ad), ad + bd)
    if k == "mul":
        return (an + bn, ad + bd)
    if k == "div":
        return (an + bd, ad + bn)
    raise ValueError(k)


def _ceil_power_of_two(v):                                # src/utils.rs:76-82
    return v if v and (v & (v - 1)) == 0 else 1 << max(v, 1).bit_length() if v else 1


def constraint_blowup_factor(c, trace_len):
    """`Constraint::blowup_factor` (src/constraints.rs:162-166, 340-347) -- note the division by trace_len - 1."""
    n, d = _degree(c, trace_len - 1)
    return _ceil_power_of_two(max(n - d, 0)) // (trace_len - 1)


def composition_constraint(trace_len, constraints, num_air_challenges=0, min_ce_blowup=1):
    """`AirConfig::composition_constraint` (src/air.rs:50-82): sum_i c_i (X^adj_i alpha_i + beta_i) with
    adj_i = (trace_len ce_blowup - 1) - (deg num_i - deg den_i).  CompositionCoeff(i) is Challenge(num_air_challenges + i) here: the AIR's own
    challenges come first, as `prove` draws them first (eval_constraint substitutes both as constants, src/air.rs:96-101).
    min_ce_blowup: a floor for the constraint-evaluation blow-up.  Returns (expression, ce_blowup_factor, number of composition coefficients)."""
    ce = max(min_ce_blowup, max(constraint_blowup_factor(c, trace_len) for c in constraints))
    composition_degree = trace_len * ce - 1
    x = E.X()
    comp = None
    for i, c in enumerate(constraints):
        n, d = _degree(c, trace_len - 1)
        assert n - d <= composition_degree
        adj = composition_degree - (n - d)
        term = c * (x ** adj * E.Challenge(num_air_challenges + 2 * i) + E.Challenge(num_air_challenges + 2 * i + 1))
        comp = term if comp is None else comp + term
    return comp, ce, 2 * len(constraints)


def fib_air_constraints(trace_len, field=GOLDILOCKS_FP):
    """`FibAirConfig::constraints` (examples/fib/main.rs:73-140), in its order: 8 boundary constraints divided by (X - 1),
    the terminal constraint divided by (X - g^-1), 8 multiplicative transition constraints times (X - g^-1) / (X^n - 1).
    Hint(0) is the claimed n-th value.  field: the base field the trace domain lives in (the example's is Goldilocks;
    src/eval_gpu.rs:1054-1082 runs its evaluator over the 252-bit field as well)."""
    x = E.X()
    dom = Radix2EvaluationDomain(trace_len, 1, field)
    first_x, last_x = 1, pow(dom.group_gen, trace_len - 1, dom.p)
    curr, nxt = (lambda k: E.Trace(k, 0)), (lambda k: E.Trace(k, 1))
    v = [1, 2, 2]
    for k in range(3, 8):
        v.append(v[k - 2] * v[k - 1] % dom.p)                      # 4, 8, 32, 256, 8192
    boundary = [(curr(k) - E.Constant(v[k])) / (x - E.Constant(first_x)) for k in range(8)]
    terminal = [(curr(7) - E.Hint(0)) / (x - E.Constant(last_x))]
    tr = [nxt(0) - curr(6) * curr(7), nxt(1) - curr(7) * nxt(0)] + [nxt(k) - nxt(k - 2) * nxt(k - 1) for k in range(2, 8)]
    zer = (x - E.Constant(last_x)) / (x ** trace_len - E.Constant(1))
    return boundary + terminal + [t * zer for t in tr]


def fib_constraints(n_trace, ncols=8, field=GOLDILOCKS_FP):
    """The reference's fib AIR as `default_prove` sees it: (composition constraint, ce_blowup_factor, number of composition
    coefficients).  ce_blowup_factor is 1 for this AIR (every constraint has evaluation degree <= n - 1), i.e. the
    composition polynomial has n coefficients and one column (src/prover.rs:111-124)."""
    assert ncols == 8, "examples/fib has 8 columns"
    return composition_constraint(n_trace, fib_air_constraints(n_trace, field))


PERMUTATION_ROTATION = 5


def permutation_trace(n, seed):
    """A valid base trace of `permutation_air`: columns x0, x1, y0, y1 as canonical integers.  The y rows of 0..n-2 are the x rows of 0..n-2
    cyclically rotated by PERMUTATION_ROTATION; row n-1 is padding (the running products stop in front of it)."""
    rng = np.random.default_rng(seed)
    x = [[int(v) for v in rng.integers(0, GL_P, size=n, dtype=np.uint64)] for _ in range(2)]
    pad = [int(v) for v in rng.integers(0, GL_P, size=2, dtype=np.uint64)]
    m = n - 1
    y = [[col[(i + PERMUTATION_ROTATION) % m] for i in range(m)] + [pad[k]] for k, col in enumerate(x)]
    return x + y


SORTED_PERMUTATION_X0_RANGE = 16


def sorted_permutation_trace(n, seed):
    """A valid base trace of `permutation_air`, built on the host: x0 drawn from 0..15 (so rows tie on it), x1 at random, and the y rows of
    0..n-2 the x rows of 0..n-2 sorted by (x0, x1) -- the order of a memory table; row n-1 is padding.  Canonical integers."""
    rng = np.random.default_rng(seed)
    x0 = [int(v) for v in rng.integers(0, SORTED_PERMUTATION_X0_RANGE, size=n)]
    x1 = [int(v) for v in rng.integers(0, GL_P, size=n, dtype=np.uint64)]
    pad = [int(v) for v in rng.integers(0, GL_P, size=2, dtype=np.uint64)]
    order = sorted(range(n - 1), key=lambda i: (x0[i], x1[i]))
    return [x0, x1, [x0[i] for i in order] + [pad[0]], [x1[i] for i in order] + [pad[1]]]


def sorted_permutation_trace_on_device(planner, n, seed):
    """`sorted_permutation_trace(n, seed)` with its y columns ordered where the trace lies: x0 and x1 are uploaded, ms_sort_rows
    (extension.sort_rows) sorts rows 0..n-2 by (x0, x1), ms_permute_columns (extension.permute_columns) gathers them into y0 and y1, and the
    padding row n-1 is written behind them -- no download, no host sort.  -> the base trace as a Matrix of four Fp columns, equal to the
    uploaded `sorted_permutation_trace` in every word; `permutation_air(n)` is valid on it."""
    from .api import GpuVec
    from .extension import SortKey, permute_columns, sort_rows
    rng = np.random.default_rng(seed)
    x0 = rng.integers(0, SORTED_PERMUTATION_X0_RANGE, size=n)
    x1 = rng.integers(0, GL_P, size=n, dtype=np.uint64)
    pad = [int(v) for v in rng.integers(0, GL_P, size=2, dtype=np.uint64)]
    x = Matrix.from_numpy(planner, [to_mont_words(GOLDILOCKS_FP, [int(v) for v in c]).ravel() for c in (x0, x1)], GOLDILOCKS_FP)
    y = [GpuVec(planner, n, GOLDILOCKS_FP) for _ in range(2)]
    perm, _ = sort_rows(planner, x, SortKey([0, 1]), n=n - 1)
    permute_columns(planner, x, perm, out=y)
    L = planner.lib
    for col, v in zip(y, pad):
        w = to_mont_words(GOLDILOCKS_FP, [v]).ravel()
        L.check(L.ms_upload(planner.handle, col.ptr + 8 * (n - 1), w.ctypes.data, 8))
    return Matrix(x.columns + y)


def permutation_air_constraints(n):
    """The seven constraints of `permutation_air`, in its order: the boundaries P = 1, Q = 1, E = 0 at row 0, the terminal P = Q at row
    n-1, and the three transitions on rows 0..n-2."""
    x = E.X()
    dom = Radix2EvaluationDomain(n, 1, GOLDILOCKS_FP)
    last_x = pow(dom.group_gen, n - 1, dom.p)
    cur, nxt, ch = (lambda k: E.Trace(k, 0)), (lambda k: E.Trace(k, 1)), E.Challenge
    P, Q, EV = 4, 5, 6
    boundary = [(cur(P) - E.Constant(1)) / (x - E.Constant(1)), (cur(Q) - E.Constant(1)) / (x - E.Constant(1)), cur(EV) / (x - E.Constant(1))]
    terminal = [(cur(P) - cur(Q)) / (x - E.Constant(last_x))]
    tr = [nxt(P) - cur(P) * (ch(0) - ch(1) * cur(0) - ch(2) * cur(1)),
          nxt(Q) - cur(Q) * (ch(0) - ch(1) * cur(2) - ch(2) * cur(3)),
          nxt(EV) - (ch(3) * cur(EV) + nxt(0))]
    zer = (x - E.Constant(last_x)) / (x ** n - E.Constant(1))
    return boundary + terminal + [t * zer for t in tr]


def permutation_air(n):
    """A small AIR with an extension trace, valid on `permutation_trace`: the rows (y0, y1) are a permutation of the rows (x0, x1), shown by
    two running products over challenges drawn after the base commitment, plus a running evaluation of x0 (the three shapes of
    examples/brainfuck/trace.rs:108-289).  Base columns 0..3 = x0, x1, y0, y1; extension columns 4..6 = P, Q, E; challenges 0..3 = alpha,
    beta, gamma, delta:
        P' = P (alpha - beta x0 - gamma x1)      Q' = Q (alpha - beta y0 - gamma y1)      E' = delta E + x0'
    P = Q = 1 and E = 0 at row 0, P = Q at row n-1; the transitions hold on rows 0..n-2 (divided by (X^n - 1) / (X - g^(n-1))).
    -> (composition constraint, ce_blowup 2, number of composition coefficients, number of AIR challenges 4, the ExtColumn records)."""
    from .extension import ExtColumn
    comp, ce, ncoeffs = composition_constraint(n, permutation_air_constraints(n), num_air_challenges=4, min_ce_blowup=2)
    product = lambda c0, c1: ExtColumn(1, [(+1, 0, None), (-1, 1, c0), (-1, 2, c1)], [])
    columns = [product(0, 1), product(2, 3), ExtColumn(0, [(+1, 3, None)], [(+1, None, 0, 1)])]
    return comp, ce, ncoeffs, 4, columns


def lookup_trace(n, seed):
    """A valid base trace of `lookup_air`: columns a0, a1, t0, t1, m as canonical integers.  Every looked-up pair (a0, a1)[i] is a row of the
    table (t0, t1) and m[j] counts the rows that look table row j up.  Only the first half of the table is ever looked up, so the upper
    half has m = 0 and -- n lookups into n / 2 rows -- some row has m >= 2."""
    assert n >= 4
    rng = np.random.default_rng(seed)
    t = [[int(v) for v in rng.integers(0, GL_P, size=n, dtype=np.uint64)] for _ in range(2)]
    idx = [int(v) for v in rng.integers(0, n // 2, size=n)]
    m = [0] * n
    for j in idx:
        m[j] += 1
    return [[t[0][j] for j in idx], [t[1][j] for j in idx]] + t + [m]


def lookup_trace_on_device(planner, n, seed, check=False):
    """`lookup_trace(n, seed)` with its m column counted where the trace lies: the a and t columns are uploaded beside a zero m column and
    ms_lookup_multiplicities (extension.lookup_multiplicities) fills that column in place -- no download, no host loop, no second upload.
    -> the base trace as a Matrix of five Fp columns, equal to the uploaded `lookup_trace` in every word.  check: read the call's report
    (a host wait) and raise LookupMissing if a looked-up pair is not a row of the table."""
    from .extension import LookupTuple, lookup_multiplicities
    cols = lookup_trace(n, seed)
    trace = Matrix.from_numpy(planner, [to_mont_words(GOLDILOCKS_FP, c).ravel() for c in cols[:4]] + [np.zeros(n, dtype=np.uint64)], GOLDILOCKS_FP)
    _, report = lookup_multiplicities(planner, trace, LookupTuple([2, 3]), [LookupTuple([0, 1])], out=trace.columns[4])
    if check:
        report.check()
    return trace


def fetch_program(n, seed):
    """The program table of `fetch_trace`: L = n / 2 rows (addr, val) as canonical integers, the addresses an affine progression mod p with
    a nonzero step -- distinct by construction -- and the values drawn."""
    assert n >= 4
    rng = np.random.default_rng([seed, 1])
    start, step = (int(v) for v in rng.integers(1, GL_P, size=2, dtype=np.uint64))
    L = n // 2
    return [[(start + j * step) % GL_P for j in range(L)], [int(v) for v in rng.integers(0, GL_P, size=L, dtype=np.uint64)]]


def fetch_trace(n, seed, program=None):
    """A valid base trace of `lookup_air` whose looked-up VALUES are fetched: columns a0, a1, t0, t1, m as canonical integers.  The program
    (`fetch_program(n, seed)` unless one is given) is a table of n / 2 rows (addr, val) with distinct addresses; t0, t1 are the program
    padded to n rows by repeating its last row (the repeated rows are duplicates of it: m = 0); a0 is n addresses drawn from the program,
    a1[i] the value the program holds at a0[i] -- an instruction fetch -- and m[j] counts the rows that read program row j."""
    addr, val = fetch_program(n, seed) if program is None else program
    L = len(addr)
    rng = np.random.default_rng([seed, 2])
    idx = [int(v) for v in rng.integers(0, L, size=n)]
    m = [0] * n
    for j in idx:
        m[j] += 1
    pad = lambda c: list(c) + [c[-1]] * (n - L)
    return [[addr[j] for j in idx], [val[j] for j in idx], pad(addr), pad(val), m]


def fetch_trace_on_device(planner, n, seed, check=False, a0=None):
    """`fetch_trace(n, seed)` built where the trace lies: a0, the program and t0, t1 are uploaded; a1 is FETCHED -- ms_join_rows finds, for
    every a0[i], the program row that holds that address and ms_permute_columns reads its value (extension.fetch_columns, into the trace's
    own a1 column) -- and ms_lookup_multiplicities fills m in place.  Nothing is downloaded.
    -> the base trace as a Matrix of five Fp columns, equal to the uploaded `fetch_trace` in every word.  check: read both calls' reports
    (host waits) and raise LookupMissing if an address is not in the program, or a looked-up pair is not a row of the table.
    a0: the addresses to fetch, in place of the drawn ones (canonical integers)."""
    from .extension import LookupTuple, fetch_columns, lookup_multiplicities
    program = fetch_program(n, seed)
    cols = fetch_trace(n, seed, program)
    words = lambda c: to_mont_words(GOLDILOCKS_FP, c).ravel()
    zero = np.zeros(n, dtype=np.uint64)
    d_program = Matrix.from_numpy(planner, [words(c) for c in program], GOLDILOCKS_FP)
    trace = Matrix.from_numpy(planner, [words(cols[0] if a0 is None else a0), zero, words(cols[2]), words(cols[3]), zero], GOLDILOCKS_FP)
    fetch_columns(planner, d_program, LookupTuple([0]), trace, LookupTuple([0]), [1], out=[trace.columns[1]], check=check)
    _, report = lookup_multiplicities(planner, trace, LookupTuple([2, 3]), [LookupTuple([0, 1])], out=trace.columns[4])
    if check:
        report.check()
    return trace


def lookup_air_constraints(n):
    """The two constraints of `lookup_air`, in its order: the boundary S = 0 at row 0, and the transition over the full zerofier X^n - 1."""
    x = E.X()
    cur, nxt, ch = (lambda k: E.Trace(k, 0)), (lambda k: E.Trace(k, 1)), E.Challenge
    S = 5
    dt, da = ch(0) - cur(2) - ch(1) * cur(3), ch(0) - cur(0) - ch(1) * cur(1)
    return [cur(S) / (x - E.Constant(1)), ((nxt(S) - cur(S)) * dt * da - cur(4) * da + dt) / (x ** n - E.Constant(1))]


def lookup_air(n):
    """A small AIR with a logarithmic-derivative lookup (LogUp), valid on `lookup_trace`: every pair (a0, a1) is a row of the table (t0, t1),
    which is looked up m times.  Base columns 0..4 = a0, a1, t0, t1, m; extension column 5 = S; challenges 0, 1 = alpha, beta:
        S' = S + m / Dt - 1 / Da,      Dt = alpha - t0 - beta t1,      Da = alpha - a0 - beta a1
    S = 0 at row 0, and the transition, cleared of its denominators, (S' - S) Dt Da - m Da + Dt = 0 on EVERY row (divided by X^n - 1):
    Trace(S, 1) of the last row is S of row 0, so the wrap-around is the statement that the fractions sum to zero and there is no terminal
    constraint.
    -> (composition constraint, ce_blowup, number of composition coefficients, number of AIR challenges 2, the LogUpColumn record)."""
    from .extension import LogUpColumn
    comp, ce, ncoeffs = composition_constraint(n, lookup_air_constraints(n), num_air_challenges=2)
    den = lambda c0, c1: [(+1, 0, None), (-1, None, c0), (-1, 1, c1)]
    columns = [LogUpColumn(0, [([(+1, None, 4)], den(2, 3)), ([(-1, None, None)], den(0, 1))])]
    return comp, ce, ncoeffs, 2, columns


def range_trace(n, bits, seed):
    """A valid base trace of `range_air`: columns x, l0, l1, t, m as canonical integers.  x is drawn below 2^(2 bits), l0 and l1 are its
    low and high limbs of `bits` bits, t[j] = min(j, 2^bits - 1) is the table 0 .. 2^bits - 1 padded to n rows by repeating its last row,
    and m[j] counts how often j occurs in l0 and l1 together (zero from 2^bits on).  n >= 2^bits."""
    assert 1 <= bits <= 16 and n >= (1 << bits)
    rng = np.random.default_rng(seed)
    x = [int(v) for v in rng.integers(0, 1 << (2 * bits), size=n, dtype=np.uint64)]
    l0, l1 = [v & ((1 << bits) - 1) for v in x], [v >> bits for v in x]
    m = [0] * n
    for v in l0 + l1:
        m[v] += 1
    return [x, l0, l1, [min(j, (1 << bits) - 1) for j in range(n)], m]


def range_trace_on_device(planner, n, bits, seed, check=False, x=None):
    """`range_trace(n, bits, seed)` built where the trace lies: x and t are uploaded beside three zero columns, ms_limb_decompose
    (extension.limb_decompose) writes l0 and l1, and ms_range_multiplicities (extension.range_multiplicities) counts both limb columns into
    m in place -- by direct indexing: t is a column of the AIR, not an input of the count.  Nothing is downloaded.
    -> the base trace as a Matrix of five Fp columns, equal to the uploaded `range_trace` in every word.  check: read both calls' reports
    (host waits) and raise LookupMissing if a value does not fit two limbs, or a limb is not below 2^bits.
    x: the values to decompose, in place of the drawn ones (canonical integers)."""
    from .extension import LimbSpec, RangeSet, limb_decompose, range_multiplicities
    cols = range_trace(n, bits, seed)
    words = lambda c: to_mont_words(GOLDILOCKS_FP, c).ravel()
    zero = np.zeros(n, dtype=np.uint64)
    trace = Matrix.from_numpy(planner, [words(cols[0] if x is None else x), zero, zero, words(cols[3]), zero], GOLDILOCKS_FP)
    limbs = limb_decompose(planner, trace, [LimbSpec(0, 1, 2, bits)])
    _, counts = range_multiplicities(planner, trace, bits, [RangeSet(1), RangeSet(2)], out=trace.columns[4])
    if check:
        limbs.check()
        counts.check()
    return trace


def range_air_constraints(n, bits):
    """The three constraints of `range_air`, in its order: the recomposition x = l0 + 2^bits l1 on every row, the boundary S = 0 at row 0,
    and the LogUp transition, both transitions over the full zerofier X^n - 1."""
    x = E.X()
    cur, nxt, ch = (lambda k: E.Trace(k, 0)), (lambda k: E.Trace(k, 1)), E.Challenge
    S = 5
    zerofier = x ** n - E.Constant(1)
    dt, d0, d1 = ch(0) - cur(3), ch(0) - cur(1), ch(0) - cur(2)
    return [(cur(0) - cur(1) - E.Constant(1 << bits) * cur(2)) / zerofier,
            cur(S) / (x - E.Constant(1)),
            ((nxt(S) - cur(S)) * dt * d0 * d1 - cur(4) * d0 * d1 + dt * d1 + dt * d0) / zerofier]


def range_air(n, bits):
    """A range-checked AIR, valid on `range_trace`: x is two limbs of `bits` bits, and both limbs are rows of the table t = 0 .. 2^bits - 1,
    which is looked up m times.  Base columns 0..4 = x, l0, l1, t, m; extension column 5 = S; challenge 0 = alpha:
        x - l0 - 2^bits l1 = 0,        S' = S + m / (alpha - t) - 1 / (alpha - l0) - 1 / (alpha - l1)
    S = 0 at row 0, and the transition, cleared of its three denominators, on EVERY row (divided by X^n - 1): Trace(S, 1) of the last row is S
    of row 0, so the wrap-around is the statement that the fractions sum to zero and there is no terminal constraint, as in `lookup_air`.
    The cleared transition has degree 4: ce_blowup comes out as 4, so `prove` needs blowup >= 4.
    -> (composition constraint, ce_blowup, number of composition coefficients, number of AIR challenges 1, the LogUpColumn record)."""
    from .extension import LogUpColumn
    comp, ce, ncoeffs = composition_constraint(n, range_air_constraints(n, bits), num_air_challenges=1)
    den = lambda c: [(+1, 0, None), (-1, None, c)]
    columns = [LogUpColumn(0, [([(+1, None, 4)], den(3)), ([(-1, None, None)], den(1)), ([(-1, None, None)], den(2))])]
    return comp, ce, ncoeffs, 1, columns


_BITWISE = {"and": (0, lambda x, y: x & y), "or": (1, lambda x, y: x | y), "xor": (2, lambda x, y: x ^ y)}
BITWISE_COLUMNS = ("a", "b", "c", "a0", "a1", "b0", "b1", "c0", "c1", "tx", "ty", "tz", "m")


def bitwise_trace(n, bits, op, seed):
    """A valid base trace of `bitwise_air`: columns a, b, c, a0, a1, b0, b1, c0, c1, tx, ty, tz, m as canonical integers.  a and b are
    drawn below 2^(2 bits), c = a op b (op "and", "or" or "xor"), x0 and x1 are the low and high limbs of `bits` bits of x, (tx, ty, tz) is
    the table (x, y, x op y) over all pairs of limbs -- row x * 2^bits + y -- padded to n rows by repeating its last row, and m[j] counts
    how often table row j is the limb triple (a_k, b_k, c_k) of a row, k = 0, 1 (zero from 4^bits on).  n >= 4^bits."""
    assert 1 <= bits <= 8 and n >= (1 << (2 * bits)) and op in _BITWISE
    fn, lm, T = _BITWISE[op][1], (1 << bits) - 1, 1 << (2 * bits)
    rng = np.random.default_rng(seed)
    a = [int(v) for v in rng.integers(0, T, size=n, dtype=np.uint64)]
    b = [int(v) for v in rng.integers(0, T, size=n, dtype=np.uint64)]
    c = [fn(x, y) for x, y in zip(a, b)]
    limbs = [[v & lm for v in col] if k == 0 else [v >> bits for v in col] for col in (a, b, c) for k in (0, 1)]
    rows = [min(j, T - 1) for j in range(n)]
    tx, ty = [r >> bits for r in rows], [r & lm for r in rows]
    m = [0] * n
    for k in (0, 1):
        for x, y in zip(limbs[k], limbs[2 + k]):
            m[(x << bits) + y] += 1
    return [a, b, c] + limbs + [tx, ty, [fn(x, y) for x, y in zip(tx, ty)], m]


def bitwise_trace_on_device(planner, n, bits, op, seed, check=False, a=None, b=None, c=None):
    """`bitwise_trace(n, bits, op, seed)` built where the trace lies: a and b are uploaded beside eleven zero columns, ms_bitwise_columns
    (extension.bitwise_columns) writes c, one ms_limb_decompose writes the six limb columns, ms_bitwise_table writes tx, ty, tz and
    ms_bitwise_multiplicities counts the limb pairs of (a, b), checked against c, into m in place -- from the word columns: the limb columns
    are columns of the AIR, not inputs of the count.  Nothing is downloaded.
    -> the base trace as a Matrix of thirteen Fp columns, equal to the uploaded `bitwise_trace` in every word.  check: read the three
    reports (host waits) and raise LookupMissing if an operand does not fit two limbs or c is not a op b.
    a, b: the operands, in place of the drawn ones (canonical integers).  c: a result column uploaded in place of the one
    ms_bitwise_columns would write -- the negative control of a prover that got it wrong."""
    from .extension import BitwiseSet, BitwiseSpec, LimbSpec, bitwise_columns, bitwise_multiplicities, bitwise_table, limb_decompose
    cols = bitwise_trace(n, bits, op, seed)
    words = lambda c: to_mont_words(GOLDILOCKS_FP, c).ravel()
    zero = np.zeros(n, dtype=np.uint64)
    trace = Matrix.from_numpy(planner, [words(cols[0] if a is None else a), words(cols[1] if b is None else b), zero if c is None else words(c)] + [zero] * 10, GOLDILOCKS_FP)
    made = bitwise_columns(planner, trace, [BitwiseSpec(op, 0, 1, 2, 2 * bits)] if c is None else [])
    limbs = limb_decompose(planner, trace, [LimbSpec(src, 3 + 2 * src, 2, bits) for src in range(3)])
    bitwise_table(planner, GOLDILOCKS_FP, bits, [op], n_t=n, out=[None] + trace.columns[9:12])
    _, counts = bitwise_multiplicities(planner, trace, bits, [op], [BitwiseSet(op, 0, 1, 2, 2)], out=trace.columns[12])
    if check:
        made.check()
        limbs.check()
        counts.check()
    return trace


def bitwise_air_constraints(n, bits):
    """The five constraints of `bitwise_air`, in its order: the recompositions x = x0 + 2^bits x1 of a, b and c on every row, the boundary
    S = 0 at row 0, and the LogUp transition, the transitions over the full zerofier X^n - 1."""
    x = E.X()
    cur, nxt, ch = (lambda k: E.Trace(k, 0)), (lambda k: E.Trace(k, 1)), E.Challenge
    S = 13
    zerofier = x ** n - E.Constant(1)
    den = lambda cx, cy, cz: ch(0) - cur(cx) - ch(1) * cur(cy) - ch(2) * cur(cz)
    dt, d0, d1 = den(9, 10, 11), den(3, 5, 7), den(4, 6, 8)
    return [(cur(src) - cur(3 + 2 * src) - E.Constant(1 << bits) * cur(4 + 2 * src)) / zerofier for src in range(3)] + [
            cur(S) / (x - E.Constant(1)),
            ((nxt(S) - cur(S)) * dt * d0 * d1 - cur(12) * d0 * d1 + dt * d1 + dt * d0) / zerofier]


def bitwise_air(n, bits, op):
    """An AIR of a bitwise operation, valid on `bitwise_trace`: a, b and c are two limbs of `bits` bits each, and both limb triples
    (a_k, b_k, c_k) are rows of the table (tx, ty, tz) = (x, y, x op y), which is looked up m times.  Base columns 0..12 = a, b, c, a0, a1,
    b0, b1, c0, c1, tx, ty, tz, m; extension column 13 = S; challenges 0, 1, 2 = alpha, beta1, beta2:
        x - x0 - 2^bits x1 = 0  for x = a, b, c
        S' = S + m / (alpha - tx - beta1 ty - beta2 tz) - sum_k 1 / (alpha - a_k - beta1 b_k - beta2 c_k)
    S = 0 at row 0, and the transition, cleared of its three denominators, on EVERY row (divided by X^n - 1), as in `range_air`: degree 4,
    ce_blowup 4.  `op` is in the table column tz alone: the constraints are the same for the three ops.
    -> (composition constraint, ce_blowup, number of composition coefficients, number of AIR challenges 3, the LogUpColumn record)."""
    from .extension import LogUpColumn
    assert op in _BITWISE
    comp, ce, ncoeffs = composition_constraint(n, bitwise_air_constraints(n, bits), num_air_challenges=3)
    den = lambda cx, cy, cz: [(+1, 0, None), (-1, None, cx), (-1, 1, cy), (-1, 2, cz)]
    columns = [LogUpColumn(0, [([(+1, None, 12)], den(9, 10, 11)), ([(-1, None, None)], den(3, 5, 7)), ([(-1, None, None)], den(4, 6, 8))])]
    return comp, ce, ncoeffs, 3, columns


def memory_processor_rows(steps, seed):
    """The processor table of a small tape machine, as canonical integers: columns cycle, mp, mem_val, instr; `steps` executed rows and the
    final state row, whose instr is 0.  Instructions 1..4, drawn at random: increment and decrement the cell under the pointer (mod p), move
    the pointer right, move it left (at address 0 it stays).  mem_val is the cell's value BEFORE the instruction, as in
    examples/brainfuck/vm.rs."""
    rng = np.random.default_rng(seed)
    instrs = [int(v) for v in rng.integers(1, 5, size=steps)] + [0]
    mem, mp, rows = {}, 0, []
    for cycle, ins in enumerate(instrs):
        rows.append((cycle, mp, mem.get(mp, 0), ins))
        if ins == 1:
            mem[mp] = (mem.get(mp, 0) + 1) % GL_P
        elif ins == 2:
            mem[mp] = (mem.get(mp, 0) - 1) % GL_P
        elif ins == 3:
            mp += 1
        elif ins == 4:
            mp = max(mp - 1, 0)
    return [[r[c] for r in rows] for c in range(4)]


def memory_table_trace(steps, seed):
    """The memory table of `memory_processor_rows(steps, seed)`, derived on the host as examples/brainfuck/vm.rs does (derive_memory_rows,
    pad_memory_rows): the rows whose instr is not 0, sorted by (mp, cycle); a dummy row for every cycle missing between two rows of one
    address; the last row repeated, its clock running on and dummy set, up to the least power of two.  -> columns cycle, mp, mem_val, dummy as
    canonical integers."""
    cycle, mp, val, ins = memory_processor_rows(steps, seed)
    rows = sorted((mp[i], cycle[i], val[i]) for i in range(len(ins)) if ins[i] != 0)
    out = []
    for k, (a, c, v) in enumerate(rows):
        out.append((c, a, v, 0))
        if k + 1 < len(rows) and rows[k + 1][0] == a:
            out += [(t, a, v, 1) for t in range(c + 1, rows[k + 1][1])]
    n = 1
    while n < len(out):
        n *= 2
    while len(out) < n:
        c, a, v, _ = out[-1]
        out.append(((c + 1) % GL_P, a, v, 1))
    return [[r[c] for r in out] for c in range(4)]


def memory_table_trace_on_device(planner, steps, seed, check=False):
    """`memory_table_trace(steps, seed)` built where the processor table lies: its four columns are uploaded, ms_sort_rows
    (extension.sort_rows) orders the rows whose instr is not 0 by (mp, cycle), ms_gap_plan (extension.gap_plan) goes through that permutation
    with the same mask and counts, per row, the cycles missing up to the next row of its address, and ms_gap_fill (extension.gap_fill)
    writes cycle (a counter), mp and mem_val (copies) and dummy (a flag), padded to the least power of two -- the table is never
    downloaded; the one host wait reads the row count to size the result.  check: raise extension.GapError if a clock does not ascend.
    -> a Matrix of four Fp columns, equal to the uploaded `memory_table_trace` in every word; `memory_air` is valid on it."""
    from .extension import GapSpec, SortKey, gap_fill, gap_plan, sort_rows
    proc = Matrix.from_numpy(planner, [to_mont_words(GOLDILOCKS_FP, c).ravel() for c in memory_processor_rows(steps, seed)], GOLDILOCKS_FP)
    perm, _ = sort_rows(planner, proc, SortKey([1, 0], mask=("nonzero", 3)))
    plan = gap_plan(planner, proc, GapSpec(group=[1], counter=0, mask=("nonzero", 3)), perm=perm)
    if check:
        plan.report.check()
    return gap_fill(planner, proc, plan, [("counter", 0), ("copy", 1), ("copy", 2), ("flag", None)])


def memory_air_constraints(n):
    """The constraints of the reference's memory table (examples/brainfuck/constraints.rs:279-309) over columns 0..3 = cycle, mp, mem_val,
    dummy, in its order: the boundaries cycle = mp = mem_val = 0 at row 0 and the six transitions on rows 0..n-2:
        (mp' - mp - 1)(mp' - mp)      (mp' - mp) mem_val'      (dummy' - 1) dummy'      (mp' - mp) dummy      (mem_val' - mem_val) dummy
        (mp' - mp - 1)(cycle' - cycle - 1)"""
    x = E.X()
    dom = Radix2EvaluationDomain(n, 1, GOLDILOCKS_FP)
    last_x = pow(dom.group_gen, n - 1, dom.p)
    cur, nxt, one = (lambda k: E.Trace(k, 0)), (lambda k: E.Trace(k, 1)), E.Constant(1)
    CYCLE, MP, VAL, DUMMY = 0, 1, 2, 3
    boundary = [cur(c) / (x - one) for c in (CYCLE, MP, VAL)]
    step = nxt(MP) - cur(MP)
    tr = [(step - one) * step, step * nxt(VAL), (nxt(DUMMY) - one) * nxt(DUMMY), step * cur(DUMMY), (nxt(VAL) - cur(VAL)) * cur(DUMMY),
          (step - one) * (nxt(CYCLE) - cur(CYCLE) - one)]
    zer = (x - E.Constant(last_x)) / (x ** n - one)
    return boundary + [t * zer for t in tr]


def memory_air(n):
    """The AIR of `memory_air_constraints` as `prove` takes it, valid on `memory_table_trace`: -> (composition constraint, ce_blowup, number
    of composition coefficients).  It has no extension trace and no challenges of its own."""
    return composition_constraint(n, memory_air_constraints(n))


def additive_constraints(n_trace, ncols=8, ce_blowup=4):
    """A second, cheaper shape (the round-1/2 stand-in, kept as an extra case): additive transitions c_k = c_(k-2) + c_(k-1),
    each times (X - 3) / (X^n - 1) and (alpha_k X^3 + beta_k), evaluated on a constraint-evaluation domain of `ce_blowup` n points."""
    x = E.X()
    c = [lambda o=0, k=k: E.Trace(k, o) for k in range(ncols)]
    cons = [c[0](1) - (c[ncols - 2]() + c[ncols - 1]()), c[1](1) - (c[ncols - 1]() + c[0](1))]
    cons += [c[k]() - (c[k - 2]() + c[k - 1]()) for k in range(2, ncols)]
    zer = (x - E.Constant(3)) / (x ** n_trace - 1)
    comp = None
    for k, cn in enumerate(cons):
        term = cn * zer * (E.Challenge(2 * k) * x ** 3 + E.Challenge(2 * k + 1))
        comp = term if comp is None else comp + term
    return comp, ce_blowup, 2 * len(cons)


def mixed_air_constraints():
    """A 17 Fp + 9 Fq3-column composition in the shape of the brainfuck AIR (examples/brainfuck/air.rs:26-27, 68-125:
    running-product style extension columns driven by base columns and challenges, transition zerofier (X - 1) / (X^64 - 1),
    one boundary-style term divided by (X - 3)); 4 Fq3 challenges.  -> (expression, number of challenges)."""
    x = E.X()
    b = [lambda o=0, k=k: E.Trace(k, o) for k in range(17)]
    e = [lambda o=0, k=k: E.Trace(17 + k, o) for k in range(9)]
    expr = None
    for k in range(9):
        t = (e[k](1) - e[k]() * (E.Challenge(k % 4) - b[k]() * E.Challenge((k + 1) % 4) - b[k + 8](1))) * (x - 1) / (x ** 64 - 1)
        expr = t if expr is None else expr + t * E.Challenge(k % 4)
    expr = expr + (b[16]() ** 2 - b[16]()) * e[0]() / (x - E.Constant(3))
    return expr, 4


def field_modulus(field):
    return F252_P if field == STARK252_FP else GL_P


def field_generator(field):
    """the coset offset of the LDE domain: the field's multiplicative generator (7 for Goldilocks, 3 for the 252-bit field)"""
    return 3 if field == STARK252_FP else 7


def to_mont_words(field, values):
    """canonical integers of the base field -> their Montgomery words, one row per element (1 word, or 4 for the 252-bit field)"""
    if field == STARK252_FP:
        return np.array([f252_to_mont_limbs(int(v) % F252_P) for v in values], dtype=np.uint64).reshape(-1, 4)
    return np.array([gl_to_mont(v) for v in values], dtype=np.uint64).reshape(-1, 1)


class Draws:
    """What the verifier's coin would supply, fixed up front (canonical integers of Fp).  modulus: the field the draws are made
    under (the Goldilocks prime by default; its draws are what they always were)."""

    def __init__(self, seed, ncols, nchallenges, ce_blowup, nqueries, n_lde, nlayers, modulus=GL_P):
        rng = np.random.default_rng(seed)
        if modulus == GL_P:
            r = lambda k: [int(v) for v in rng.integers(1, GL_P, size=k, dtype=np.uint64)]
        else:
            r = lambda k: [1 + int.from_bytes(rng.bytes(40), "little") % (modulus - 1) for _ in range(k)]
        self.challenges = r(nchallenges)                                        # the composition coefficients (alpha_i, beta_i)
        self.hints = r(1)                                                       # FibHint::ClaimedNthFibNum
        self.z = r(1)[0]
        self.trace_args = [(c, o) for c in range(ncols) for o in (0, 1)]        # every column at the current and the next row
        self.deep = DeepCompositionCoeffs(r(len(self.trace_args)), r(ce_blowup), (r(1)[0], r(1)[0]))
        self.fri_alphas = r(nlayers)
        self.positions = [int(p) for p in rng.integers(0, n_lde, size=nqueries)]


def fold_positions(positions, folding_factor):
    """`fold_positions` (src/fri.rs:615-622): strictly increasing positions -> their cosets, deduplicated."""
    assert all(a < b for a, b in zip(positions, positions[1:]))
    out = []
    for p in positions:
        if not out or out[-1] != p // folding_factor:
            out.append(p // folding_factor)
    return out


def fri_layer_rows_launch(layer, folding_factor, positions, batch=None):
    """Rows `positions` of `Matrix::from_arrays(evaluations.as_chunks::<N>())` (src/fri.rs:213-215): N consecutive
    evaluations each, gathered on the device (32-byte records of ms_gather_digests).  Returns a function that downloads
    them as numpy [len(positions), N * words]."""
    from .api import FIELD_WORDS, DeviceBytes
    pl = layer.planner
    words = folding_factor * FIELD_WORDS[layer.field]
    if words % 4:
        return lambda: layer.to_numpy().reshape(-1, words)[positions]      # rows shorter than a 32-byte record: tiny layers only
    per = words // 4
    ids = (np.asarray(positions, dtype=np.uint64)[:, None] * np.uint64(per) + np.arange(per, dtype=np.uint64)).ravel()
    from .api import _gather_slot
    ptr, read, keep = _gather_slot(pl, 32 * len(ids), batch)
    nrec = len(layer) * FIELD_WORDS[layer.field] // 4
    if keep is batch and batch is not None:                    # a slice of the batch: joins its one launch (GatherBatch.flush)
        if ids.size and int(ids.max()) >= nrec:
            raise IndexError(f"row {int(ids.max()) // per} out of range")
        batch.defer_digests(layer.ptr, nrec, ids, ptr)
    else:
        pl.lib.check(pl.lib.ms_gather_digests(pl.handle, nrec, layer.ptr, ids.ctypes.data, len(ids), ptr))
    return lambda _keep=keep: np.array(read()[: 32 * len(ids)]).view(np.uint64).reshape(len(positions), words)


def fri_layer_rows(layer, folding_factor, positions):
    return fri_layer_rows_launch(layer, folding_factor, positions)()


def fri_num_layers(n_lde, blowup, folding, max_remainder_coeffs):
    """FriOptions::num_layers (src/fri.rs:49-56)."""
    layers, n = 0, n_lde
    while n > max_remainder_coeffs * blowup:
        n //= folding
        layers += 1
    return layers


_LOWERED = {}


def _lowered(comp_expr, ncols, field=GOLDILOCKS_FP, fq_is_ext=False):
    """The register program of an AIR's composition constraint, lowered once per expression object (an AIR's constraints are fixed; the
    C++ example compiles its program outside the proof loop as well).  Keyed by identity: the expression is kept alive by the entry."""
    key = (id(comp_expr), ncols, field, fq_is_ext)
    hit = _LOWERED.get(key)
    if hit is None or hit[0] is not comp_expr:
        if len(_LOWERED) > 16:
            _LOWERED.clear()
        hit = (comp_expr, E.compile_expr(comp_expr, ncols, fq_is_ext, field))
        _LOWERED[key] = hit
    return hit[1]


def prove_phases(planner, trace, comp_expr, draws, blowup=4, folding=8, max_remainder_coeffs=64, grinding_bits=8, hash="sha256",
                 keep=False, ce_blowup=None, time_phases=True, field=GOLDILOCKS_FP):
    """trace: Matrix of Fp columns (2^k rows).  field: GOLDILOCKS_FP, or STARK252_FP (trace, draws and constraints over the 252-bit
    field, LDE offset 3; commits with "sha256", "blake2s", "blake3_256", "keccak256", "sha3_256" or the algebraic "poseidon252" -- RPO-256 absorbs Goldilocks elements,
    Poseidon elements of the 252-bit field; a Poseidon prover grinds with SHA-256 over the last root's 32 bytes, as an RPO-256 one does).  ce_blowup: the AIR's ce_blowup_factor (src/air.rs:55-59; the constraint
    evaluation domain has trace_len * ce_blowup points, the composition trace ce_blowup columns); None = the LDE blow-up.
    Returns dict(roots=..., fri_roots=[...], remainder=GpuVec, nonce=int, queries=Queries, phases_ms={...}); with keep=True
    also the intermediate device objects (for parity tests).  time_phases=False: no device wait at the phase boundaries (two of the six
    are waits the proof itself does not need: after the evaluation and after DEEP) and no `phases_ms`."""
    pl = planner
    if field not in (GOLDILOCKS_FP, STARK252_FP):
        raise ValueError("prove_phases: field must be GOLDILOCKS_FP or STARK252_FP")
    if field == STARK252_FP and hash == "rpo256":
        raise ValueError("prove_phases: RPO-256 absorbs Goldilocks elements; the 252-bit field commits with sha256, blake2s, blake3_256, keccak256 or sha3_256, "
                         "or algebraically with poseidon252")
    if field != STARK252_FP and hash == "poseidon252":
        raise ValueError("prove_phases: poseidon252 absorbs elements of the 252-bit field: it needs field=STARK252_FP (Goldilocks commits algebraically with rpo256)")
    if field == STARK252_FP and trace.field != field:
        raise ValueError("prove_phases: field=STARK252_FP needs a trace over that field")
    h = field_generator(field)
    n_t = trace.num_rows()
    n_lde = n_t * blowup
    ce_blowup = blowup if ce_blowup is None else ce_blowup
    assert ce_blowup <= blowup                                                 # src/air.rs:149
    n_ce = n_t * ce_blowup
    trace_dom, lde_dom, ce_dom = Radix2EvaluationDomain(n_t, 1, field), Radix2EvaluationDomain(n_lde, h, field), Radix2EvaluationDomain(n_ce, h, field)
    prog = _lowered(comp_expr, trace.num_cols(), field)
    ch, hints = to_mont_words(field, draws.challenges), to_mont_words(field, draws.hints)
    out, phase = {}, {}
    t = time.perf_counter()

    def lap(name):
        nonlocal t
        if not time_phases:
            return
        pl.sync()
        now = time.perf_counter()
        phase[name] = (now - t) * 1e3
        t = now

    base_polys = trace.interpolate(trace_dom)                                  # prover.rs:50
    lde_t = base_polys.bit_reversed_evaluate(lde_dom)                          # prover.rs:51
    tree_t = MerkleTree.from_matrix(lde_t, hash)                               # prover.rs:52-55
    out["base_root"] = tree_t.root()
    lap("base trace: interpolate + LDE + commit")
    # the first n_ce rows of the committed (bit-reversed) LDE are the constraint-evaluation coset in its own bit-reversed order:
    # the evaluator works on them where they lie (the reference re-orders them, bit_reverse_ce_trace, prover.rs:88-91)
    comp_evals = E.eval(prog, pl, ch, hints, ce_blowup, h, n_ce, lde_t.columns, bit_reversed=True)      # prover.rs:97-107
    lap("constraint evaluation")
    kept_evals = comp_evals.clone() if keep else None                          # the next two steps work in place
    comp_poly = Matrix([comp_evals]).bit_reverse_rows().into_polynomials(ce_dom).columns[0]             # prover.rs:111-112
    comp_polys = Matrix.from_chunks(comp_poly, ce_blowup)                      # prover.rs:113-121
    comp_lde = comp_polys.bit_reversed_evaluate(lde_dom)                       # prover.rs:122
    tree_c = MerkleTree.from_matrix(comp_lde, hash)                            # prover.rs:123-124
    out["composition_root"] = tree_c.root()
    lap("composition trace: iNTT + split + LDE + commit")
    composer = DeepPolyComposer(draws.trace_args, n_t, draws.z, base_polys, None, comp_polys)          # prover.rs:137-144
    out["ood"] = composer.get_ood_evals()                                      # prover.rs:145-146
    # prover.rs:149-152: deep_composition_poly = composer.into_deep_poly(coeffs); its bit-reversed evaluations over the LDE domain are
    # the first FRI layer.  Both committed LDEs are still resident (the queries need them), so those evaluations are computed where the
    # LDEs lie -- the quotient is a polynomial: same values -- instead of 9 coset transforms, the composition, an inverse transform and
    # an LDE (ms_deep_rows; tests/test_deep_parity.py checks it against the two-step form).  keep=True also forms the coefficients.
    deep_poly = composer.into_deep_poly(draws.deep) if keep else None
    deep = Matrix([composer.into_deep_evaluations(draws.deep, lde_t, None, comp_lde, n_lde)])
    lap("DEEP: OOD evaluations + composition + LDE")
    cur, n, roots, layers, fri_layers, fri_trees = deep.columns[0], n_lde, [], [], [], []     # fri.rs:179-231
    for alpha in draws.fri_alphas:
        tree = MerkleTree.from_fri_layer(cur, folding, hash)
        roots.append(tree.root())
        fri_layers.append(cur); fri_trees.append(tree)                        # FriLayer { merkle_tree, evaluations } (fri.rs:218-221)
        if keep:
            layers.append(cur)
        cur = apply_drp(cur, to_mont_words(field, [alpha]).ravel(), folding, 1)
        n //= folding
    out["fri_roots"], out["remainder"] = roots, cur
    # FriProver::set_remainder (fri.rs:232-248): bit_reverse, iNTT over the subgroup of the remainder's size, keep n / blowup coefficients
    rem = Matrix([cur.clone()]).bit_reverse_rows().into_polynomials(Radix2EvaluationDomain(n, 1, field)).columns[0]
    out["remainder_coeffs"] = rem.to_numpy()[: max(n // blowup, 1) * (4 if field == STARK252_FP else 1)]
    lap("FRI layers (commit + fold) + remainder")
    fine, tf = {}, time.perf_counter()

    def sub(name):                                                             # host-side split of the last phase (no synchronisation)
        nonlocal tf
        now = time.perf_counter()
        fine[name] = round((now - tf) * 1e3, 3)
        tf = now

    out["nonce"] = grind_proof_of_work(pl, roots[-1] if roots else out["composition_root"], grinding_bits,   # prover.rs:160
                                       hash=pow_hash(hash))
    sub("proof of work")
    from .api import GatherBatch
    batch = GatherBatch(pl)                                                    # every gather of the phase into one buffer: ONE download
    queries = Queries(lde_t, None, comp_lde, tree_t, None, tree_c, draws.positions, batch)                # prover.rs:163-173
    sub("trace openings: index walks + gather launches")
    # fri_prover.into_proof(&query_positions) (prover.rs:161, fri.rs:148-165): per layer the folded positions' rows and Merkle view
    pos, launched = sorted(set(int(p) for p in draws.positions)), []
    for layer, tree in zip(fri_layers, fri_trees):                            # all gathers first, then the download
        pos = fold_positions(pos, folding)
        launched.append((pos, fri_layer_rows_launch(layer, folding, pos, batch), tree.prove_launch(pos, batch)))
    sub("FRI openings: index walks + gather launches")
    batch.fetch()
    sub("wait + download")
    out["queries"] = queries.fetch()
    out["fri_openings"] = [{"positions": p, "rows": rows(), "proof": proof()} for p, rows, proof in launched]
    sub("assembly")
    out["openings_ms"] = fine
    lap("proof of work + queries")
    out["phases_ms"] = {k: round(v, 3) for k, v in phase.items()}
    if keep:
        out.update(base_polys=base_polys, lde=lde_t, comp_evals=kept_evals, comp_polys=comp_polys, comp_lde=comp_lde,
                   deep_poly=deep_poly, deep_lde=deep, fri_layers=layers)
    return out


def from_mont_words(field, words):
    """Montgomery words of base-field elements (flat) -> their canonical integers"""
    from .api import f252_from_mont_limbs, gl_from_mont
    w = np.asarray(words, dtype=np.uint64).ravel()
    if field == STARK252_FP:
        return [f252_from_mont_limbs(w[i:i + 4]) for i in range(0, len(w), 4)]
    return [gl_from_mont(int(x)) for x in w]


def fq_words(fq, values):
    """canonical values of `fq` (ints; 3-tuples or ints for Fq3, an int being embedded) -> their Montgomery words, one row per element"""
    from .api import GOLDILOCKS_FQ3
    if fq != GOLDILOCKS_FQ3:
        return to_mont_words(fq, values)
    return np.array([[gl_to_mont(c) for c in (v if isinstance(v, tuple) else (v, 0, 0))] for v in values], dtype=np.uint64).reshape(-1, 3)


def from_fq_words(fq, words):
    """Montgomery words of `fq` elements (flat) -> canonical values: ints, or 3-tuples for Fq3"""
    from .api import GOLDILOCKS_FQ3
    vals = from_mont_words(GOLDILOCKS_FP if fq == GOLDILOCKS_FQ3 else fq, words)
    return [tuple(vals[i:i + 3]) for i in range(0, len(vals), 3)] if fq == GOLDILOCKS_FQ3 else vals


def prove(planner, trace, comp_expr, nchallenges, hints, seed32, blowup=4, folding=8, max_remainder_coeffs=64, grinding_bits=8,
          num_queries=32, hash="sha256", keep=False, ce_blowup=None, field=GOLDILOCKS_FP, trace_args=None, fq=None, num_air_challenges=0,
          extension=None, coin=None):
    """The phases of `prove_phases` with every challenge drawn from the transcript: a device-resident `coin.PublicCoin` seeded with
    `seed32` (the digest of the public inputs, src/channel.rs:33-44) stands where `Draws` stood, in the reference's order
    (src/prover.rs:50-173, src/channel.rs:46-100, src/fri.rs:199-247):
        commit base trace -> draw the `num_air_challenges` challenges of the AIR     build + commit the extension trace (if any)
        draw the `nchallenges` composition coefficients                             commit composition trace -> draw z
        OOD evaluations -> reseed (execution, then composition)                     draw the DEEP coefficients (src/stark.rs:41-53)
        per FRI layer: commit -> reseed with the root -> draw alpha -> fold         remainder coefficients -> reseed
        grind -> reseed with the nonce                                              draw the query positions -> openings
    fq: the field every challenge is drawn from and the composition, DEEP and FRI phases work over: `field` (the default), or
    GOLDILOCKS_FQ3 over Goldilocks -- the reference's own choice for its Goldilocks AIRs, with or without an extension trace.
    extension: a list of `extension.ExtColumn` and `extension.LogUpColumn` records -- the columns are built by ms_build_extension_columns
    and ms_build_logup_columns from the challenges where the coin drew them, and everything up to the extension commitment is enqueued without a host wait -- or a callable
    (base_trace, challenges GpuVec) -> Matrix of `fq` columns.  The composition constraint numbers the AIR's challenges first, then the
    composition coefficients (`composition_constraint(..., num_air_challenges=k)`); trace columns are numbered base | extension.
    The FRI commit phase is enqueued without a host wait: a layer's root is absorbed where the tree builder wrote it, alpha is drawn into
    device memory and the fold reads it there (ms_fri_fold_dev); roots and alphas are downloaded once, after the remainder.  The draws the
    host itself needs (challenges and composition coefficients for the evaluator, z, DEEP coefficients) are downloaded where they are needed,
    as the reference's are.  hints: canonical integers; H of the coin: BLAKE2s for a BLAKE2s prover, else SHA-256.
    coin: None keeps that choice (`pow_hash(hash)`); "rpo256" runs the whole transcript, proof-of-work included, on the algebraic
    `coin.RpoCoin` -- it needs hash="rpo256" and a Goldilocks `field` (fq Fp or Fq3), and takes seed32 as `coin.rpo_seed` does;
    "poseidon252" does the same on `coin.PoseidonCoin` -- it needs hash="poseidon252" and field=STARK252_FP, and takes seed32 as
    `coin.poseidon_seed` does.
    Returns what prove_phases returns (without timings), plus the draws as canonical values (3-tuples when fq is Fq3): air_challenges,
    challenges (the composition coefficients), z, deep, fri_alphas, positions; `extension_root` when there is an extension trace.  keep=True
    adds the intermediate device objects of prove_phases, `ext_trace` / `ext_polys` / `ext_lde`, the coin, and `remainder_poly`: all n_rem
    coefficients of the remainder's interpolant, of which `remainder_coeffs` are the first n_rem / blowup (fri.rs:244 asserts the rest vanish)."""
    from .api import FIELD_WORDS, GOLDILOCKS_FQ3, GatherBatch, GpuVec
    from .coin import PoseidonCoin, PublicCoin, RpoCoin
    from .extension import build_extension_columns
    pl = planner
    if field not in (GOLDILOCKS_FP, STARK252_FP):
        raise ValueError("prove: field must be GOLDILOCKS_FP or STARK252_FP")
    fq = field if fq is None else fq
    if fq != field and (fq != GOLDILOCKS_FQ3 or field != GOLDILOCKS_FP):
        raise ValueError("prove: fq is the base field, or GOLDILOCKS_FQ3 over GOLDILOCKS_FP")
    if field == STARK252_FP and hash == "rpo256":
        raise ValueError("prove: RPO-256 absorbs Goldilocks elements; the 252-bit field commits with sha256, blake2s, blake3_256, keccak256 or sha3_256, "
                         "or algebraically with poseidon252")
    if field != STARK252_FP and hash == "poseidon252":
        raise ValueError("prove: poseidon252 absorbs elements of the 252-bit field: it needs field=STARK252_FP (Goldilocks commits algebraically with rpo256)")
    if trace.field != field:
        raise ValueError("prove: the trace is not over `field`")
    if coin not in (None, "rpo256", "poseidon252"):
        raise ValueError('prove: coin is None (the byte coin of `hash`), "rpo256" or "poseidon252"')
    if coin == "rpo256" and (hash != "rpo256" or field != GOLDILOCKS_FP):
        raise ValueError('prove: coin="rpo256" absorbs RPO-256 roots and Goldilocks elements: it needs hash="rpo256" and field=GOLDILOCKS_FP')
    if coin == "poseidon252" and (hash != "poseidon252" or field != STARK252_FP):
        raise ValueError('prove: coin="poseidon252" absorbs Poseidon roots and elements of the 252-bit field: it needs hash="poseidon252" and field=STARK252_FP')
    h = field_generator(field)
    n_t = trace.num_rows()
    n_lde = n_t * blowup
    ce_blowup = blowup if ce_blowup is None else ce_blowup
    assert ce_blowup <= blowup                                                 # src/air.rs:149
    n_ce = n_t * ce_blowup
    trace_dom, lde_dom, ce_dom = Radix2EvaluationDomain(n_t, 1, field), Radix2EvaluationDomain(n_lde, h, field), Radix2EvaluationDomain(n_ce, h, field)
    V = FIELD_WORDS[fq]
    coin = RpoCoin(pl, seed32) if coin == "rpo256" else PoseidonCoin(pl, seed32) if coin == "poseidon252" else PublicCoin(pl, seed32, pow_hash(hash))
    out = {}

    base_polys = trace.interpolate(trace_dom)                                  # prover.rs:50
    lde_t = base_polys.bit_reversed_evaluate(lde_dom)
    tree_t = MerkleTree.from_matrix(lde_t, hash)
    coin.reseed_digest(tree_t.root_ptr())                                      # channel.commit_base_trace
    air_ch = coin.draw(fq, num_air_challenges) if num_air_challenges else None  # air.get_challenges (prover.rs:56-58): left on the device
    ext_trace = ext_polys = ext_lde = ext_tree = None
    if extension is not None:                                                  # prover.rs:59-72
        ext_trace = extension(trace, air_ch) if callable(extension) else build_extension_columns(pl, trace, air_ch, extension, fq)
        if ext_trace.num_rows() != n_t or ext_trace.field != fq:
            raise ValueError("prove: the extension trace has as many rows as the base trace and is over `fq`")
        ext_polys = ext_trace.interpolate(trace_dom)
        ext_lde = ext_polys.bit_reversed_evaluate(lde_dom)
        ext_tree = MerkleTree.from_matrix(ext_lde, hash)
        coin.reseed_digest(ext_tree.root_ptr())                                # channel.commit_extension_trace
    nbase, next_ = trace.num_cols(), ext_trace.num_cols() if ext_trace is not None else 0
    trace_args = [(c, o) for c in range(nbase + next_) for o in (0, 1)] if trace_args is None else list(trace_args)
    coeffs = coin.draw(fq, nchallenges)                                        # the composition coefficients (stark.rs:27-39)
    ch = coeffs.to_numpy().reshape(-1, V)
    if air_ch is not None:
        ch = np.concatenate([air_ch.to_numpy().reshape(-1, V), ch])
    ext_cols = list(ext_lde.columns) if ext_lde is not None else []
    if fq == field:                                                            # Fq = Fp: the interaction columns are base columns to the evaluator
        prog = _lowered(comp_expr, nbase + next_, field)
        comp_evals = E.eval(prog, pl, ch, fq_words(fq, hints), ce_blowup, h, n_ce, lde_t.columns + ext_cols, bit_reversed=True)
    else:
        prog = _lowered(comp_expr, nbase, field, True)
        comp_evals = E.eval(prog, pl, ch, fq_words(fq, hints), ce_blowup, h, n_ce, lde_t.columns, ext_cols, bit_reversed=True)
    kept_evals = comp_evals.clone() if keep else None
    comp_poly = Matrix([comp_evals]).bit_reverse_rows().into_polynomials(ce_dom).columns[0]
    comp_polys = Matrix.from_chunks(comp_poly, ce_blowup)
    comp_lde = comp_polys.bit_reversed_evaluate(lde_dom)
    tree_c = MerkleTree.from_matrix(comp_lde, hash)
    coin.reseed_digest(tree_c.root_ptr())                                      # channel.commit_composition_trace
    z = from_fq_words(fq, coin.draw(fq, 1).to_numpy())[0]                      # channel.get_ood_point
    composer = DeepPolyComposer(trace_args, n_t, z, base_polys, ext_polys, comp_polys)
    out["ood"] = composer.get_ood_evals()
    coin.reseed_elements(fq_words(fq, list(out["ood"][0]) + list(out["ood"][1])), fq)                  # channel.send_ood_evals: execution, composition
    d = from_fq_words(fq, coin.draw(fq, len(trace_args) + ce_blowup + 2).to_numpy())                   # stark.rs:41-53
    deep_coeffs = DeepCompositionCoeffs(d[: len(trace_args)], d[len(trace_args): len(trace_args) + ce_blowup], (d[-2], d[-1]))
    deep_poly = composer.into_deep_poly(deep_coeffs) if keep else None
    deep = Matrix([composer.into_deep_evaluations(deep_coeffs, lde_t, ext_lde, comp_lde, n_lde)])
    # fri.rs:179-231: nothing below waits for the device until the remainder is reseeded
    cur, n, layers, fri_trees, alphas = deep.columns[0], n_lde, [], [], []
    for _ in range(fri_num_layers(n_lde, blowup, folding, max_remainder_coeffs)):
        tree = MerkleTree.from_fri_layer(cur, folding, hash)
        coin.reseed_digest(tree.root_ptr())                                    # channel.commit_fri_layer (fri.rs:217-223)
        alpha = coin.draw(fq, 1)                                               # channel.draw_fri_alpha (fri.rs:225-227)
        layers.append(cur); fri_trees.append(tree); alphas.append(alpha)
        cur = apply_drp(cur, alpha, folding, 1)
        n //= folding
    rem = Matrix([cur.clone()]).bit_reverse_rows().into_polynomials(Radix2EvaluationDomain(n, 1, field)).columns[0]
    nrem = max(n // blowup, 1)
    coin.reseed_elements(GpuVec(pl, nrem, fq, ptr=rem.ptr))                    # channel.commit_remainder (fri.rs:232-248)
    out["base_root"], out["composition_root"] = tree_t.root(), tree_c.root()
    if ext_tree is not None:
        out["extension_root"] = ext_tree.root()
    out["fri_roots"], out["remainder"] = [t.root() for t in fri_trees], cur
    out["remainder_coeffs"] = rem.to_numpy()[: nrem * V]
    out["nonce"] = coin.grind(grinding_bits)                                   # prover.rs:160, channel.rs:76-93
    coin.reseed_int(out["nonce"])
    positions = coin.draw_queries(num_queries, n_lde)                          # channel.get_fri_query_positions (prover.rs:161)
    batch = GatherBatch(pl)
    queries = Queries(lde_t, ext_lde, comp_lde, tree_t, ext_tree, tree_c, positions, batch)             # prover.rs:163-173
    pos, launched = positions, []
    for layer, tree in zip(layers, fri_trees):
        pos = fold_positions(pos, folding)
        launched.append((pos, fri_layer_rows_launch(layer, folding, pos, batch), tree.prove_launch(pos, batch)))
    batch.fetch()
    out["queries"] = queries.fetch()
    out["fri_openings"] = [{"positions": p, "rows": rows(), "proof": proof()} for p, rows, proof in launched]
    out.update(challenges=from_fq_words(fq, coeffs.to_numpy()), z=z, deep=deep_coeffs, positions=positions, trace_args=trace_args,
               air_challenges=from_fq_words(fq, air_ch.to_numpy()) if air_ch is not None else [],
               fri_alphas=[from_fq_words(fq, a.to_numpy())[0] for a in alphas])
    if keep:
        out.update(base_polys=base_polys, lde=lde_t, comp_evals=kept_evals, comp_polys=comp_polys, comp_lde=comp_lde,
                   deep_poly=deep_poly, deep_lde=deep, fri_layers=layers, coin=coin, remainder_poly=rem)
        if ext_trace is not None:
            out.update(ext_trace=ext_trace, ext_polys=ext_polys, ext_lde=ext_lde)
    return out
