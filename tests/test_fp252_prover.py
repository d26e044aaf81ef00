"""prove_phases over the 252-bit field (fib AIR, 8 columns, offset 3), SHA-256 and BLAKE2s: what it returns is checked the way a
verifier would, in Python integers and hashlib -- the committed roots over the downloaded rows, the out-of-domain consistency of the
composition, the DEEP value at every query from the opened rows, each FRI layer's fold at the queried cosets, the remainder's degree
bound and values, the proof-of-work nonce."""
import hashlib
import sys

import numpy as np
import pytest

from tests import backends
from ministark_amd import STARK252_FP as F, Matrix, Radix2EvaluationDomain, pipeline
from ministark_amd.api import F252_P as p, f252_from_mont_limbs, f252_to_mont_limbs

BLOWUP, BITS, NQ = 4, 8, 32
CASES = [pytest.param(kind, log_t, folding, h, id=f"{kind}-2^{log_t}-fold{folding}-{h}", marks=[pytest.mark.gpu] if kind == "hip" else [])
         for kind, log_t in (("emu", 8), ("hip", 16)) for folding in (8, 4) for h in ("sha256", "blake2s")]


def _value(words):
    return f252_from_mont_limbs(np.asarray(words, dtype=np.uint64))


def _values(words):
    return [_value(r) for r in np.asarray(words, dtype=np.uint64).reshape(-1, 4)]


def _rev(v, bits):
    return int(format(v, f"0{bits}b")[::-1], 2) if bits else 0


def _lz(d):
    z = 0
    for b in d:
        if b:
            return z + 8 - b.bit_length()
        z += 8
    return z


def _root(H, rows):
    """rows: lists of canonical integers; a leaf is H over the row's elements as 32 little-endian bytes each, a node H(left || right)"""
    level = [H(b"".join(v.to_bytes(32, "little") for v in r)).digest() for r in rows]
    while len(level) > 1:
        level = [H(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
    return level[0]


def _fib_trace(n):
    """the fib AIR's trace over the 252-bit field: 8 columns, each row continues the multiplicative Fibonacci sequence 1, 2, 2, 4, 8, ..."""
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


def _eval_at(expr, x, trace_at, challenges, hints):
    """the composition constraint's expression at one out-of-domain point, in integers modulo p: Trace(c, o) from the out-of-domain
    values, x / y = x y^-1"""
    memo = {}
    ops = {"add": lambda a, b: (a + b) % p, "mul": lambda a, b: a * b % p, "div": lambda a, b: a * pow(b, -1, p) % p}

    def ev(e):
        if id(e) not in memo:
            k, a = e.kind, e.args
            if k == "x":
                r = x
            elif k == "const":
                r = a[1] % p
            elif k == "challenge":
                r = challenges[a[0]]
            elif k == "hint":
                r = hints[a[0]]
            elif k == "trace":
                r = trace_at[(a[0], a[1])]
            elif k == "neg":
                r = -ev(a[0]) % p
            elif k == "pow":
                r = pow(ev(a[0]), a[1], p)
            else:
                r = ops[k](ev(a[0]), ev(a[1]))
            memo[id(e)] = r
        return memo[id(e)]
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    return ev(expr)


@pytest.mark.parametrize("kind,log_t,folding,hash", CASES)
def test_proof_over_the_252_bit_field(kind, log_t, folding, hash):
    pl = backends.planner(kind)
    n = 1 << log_t
    N = n * BLOWUP
    cols = _fib_trace(n)
    trace = Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(v) for v in c]).astype(np.uint64) for c in cols], F)
    comp, ce, nch = pipeline.fib_constraints(n, 8, F)
    nlayers = pipeline.fri_num_layers(N, BLOWUP, folding, 64)
    draws = pipeline.Draws(252 + folding, 8, nch, ce, NQ, N, nlayers, modulus=p)
    draws.hints = [cols[7][n - 1]]
    out = pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, folding, 64, BITS, hash=hash, keep=True, ce_blowup=ce, field=F)
    H = hashlib.sha256 if hash == "sha256" else hashlib.blake2s
    assert len(out["fri_roots"]) == nlayers >= 1
    # (a) the roots, from the downloaded rows (the small size only: 2^18 rows of 8 elements through hashlib take minutes)
    if kind == "emu":
        for key, root in (("lde", out["base_root"]), ("comp_lde", out["composition_root"])):
            cs = [_values(c) for c in out[key].to_numpy()]
            assert root == _root(H, [list(r) for r in zip(*cs)]), key
        for layer, root in zip(out["fri_layers"], out["fri_roots"]):
            v = _values(layer.to_numpy())
            assert root == _root(H, [v[i:i + folding] for i in range(0, len(v), folding)])
    # (c) the nonce: the smallest one from 1 whose digest after the last FRI root has BITS leading zero bits
    nonce = 1
    while _lz(H(out["fri_roots"][-1] + nonce.to_bytes(8, "big")).digest()) < BITS:
        nonce += 1
    assert out["nonce"] == nonce
    # (b) 1. out-of-domain consistency of the composition (ce = 1: one composition column, its point z^1 = z)
    args, z = draws.trace_args, draws.z
    execution, composition = [int(v) for v in out["ood"][0]], [int(v) for v in out["ood"][1]]
    assert ce == 1 and len(composition) == 1
    assert _eval_at(comp, z, dict(zip(args, execution)), draws.challenges, draws.hints) == composition[0]
    # (b) 2. the DEEP value at every query, from the opened trace and composition rows
    q, coeffs = out["queries"], draws.deep
    g = Radix2EvaluationDomain(n, 1, F).group_gen
    w = Radix2EvaluationDomain(N, 1, F).group_gen
    log_N = N.bit_length() - 1
    layer0 = out["deep_lde"].columns[0].to_numpy().reshape(-1, 4)
    for i, pos in enumerate(draws.positions):
        x = 3 * pow(w, _rev(pos, log_N), p) % p
        acc = 0
        for j, ((col, off), ood) in enumerate(zip(args, execution)):
            acc += coeffs.execution_trace[j] * (_value(q.base_trace_values[i][4 * col:4 * col + 4]) - ood) * pow((x - z * pow(g, off, p)) % p, -1, p)
        acc += coeffs.composition_trace[0] * (_value(q.composition_trace_values[i][:4]) - composition[0]) * pow((x - z) % p, -1, p)
        assert _value(layer0[pos]) == acc % p * ((coeffs.degree[0] + coeffs.degree[1] * x) % p) % p, f"query {i} at position {pos}"
    # (b) 3. every FRI layer's fold at the queried cosets (the FRI domain is taken without its offset), then the remainder
    log_f = folding.bit_length() - 1
    wf = Radix2EvaluationDomain(folding, 1, F).group_gen
    positions = sorted(set(draws.positions))
    evaluations = [_value(layer0[pos]) for pos in positions]
    gen, size = w, N
    assert len(out["fri_openings"]) == nlayers
    for opening, alpha in zip(out["fri_openings"], draws.fri_alphas):
        folded = pipeline.fold_positions(positions, folding)
        assert opening["positions"] == folded
        rows = [_values(row) for row in opening["rows"]]
        assert [rows[folded.index(pos // folding)][pos % folding] for pos in positions] == evaluations
        nxt = []
        for row, fp in zip(rows, folded):
            offset = pow(gen, _rev(fp, (size // folding).bit_length() - 1), p)
            vals = [row[_rev(k, log_f)] for k in range(folding)]
            cs = [sum(v * pow(offset * pow(wf, k, p) % p, -j, p) for k, v in enumerate(vals)) % p for j in range(folding)]
            nxt.append(sum(c * pow(alpha, j, p) for j, c in enumerate(cs)) % p)
        evaluations, positions, gen, size = nxt, folded, pow(gen, folding, p), size // folding
    rem = _values(out["remainder_coeffs"])
    assert len(rem) == max(size // BLOWUP, 1)                          # degree <= domain_size / blowup - 1 ...
    full = _values(out["remainder"].to_numpy())                       # ... and the remainder layer IS that polynomial, at every point
    assert len(full) == size
    pts = range(size) if kind == "emu" else positions
    for pos in pts:
        x = pow(gen, _rev(pos, size.bit_length() - 1), p)
        assert sum(c * pow(x, j, p) for j, c in enumerate(rem)) % p == full[pos]
    for pos, want in zip(positions, evaluations):
        assert full[pos] == want


def test_rpo_is_refused_for_the_252_bit_field():
    pl = backends.planner("emu")
    n = 1 << 6
    cols = _fib_trace(n)
    trace = Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(v) for v in c]).astype(np.uint64) for c in cols], F)
    comp, ce, nch = pipeline.fib_constraints(n, 8, F)
    draws = pipeline.Draws(1, 8, nch, ce, 4, n * BLOWUP, 1, modulus=p)
    with pytest.raises(ValueError, match="RPO-256"):
        pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, 8, 64, BITS, hash="rpo256", ce_blowup=ce, field=F)


def test_default_arguments_still_give_the_recorded_goldilocks_proof():
    """prove_phases with default arguments (Goldilocks, SHA-256), 8 random columns of 2^8 rows on the simulator: roots, nonce and remainder
    as recorded from the commit before the field parameter existed (tests/golden/prove_phases_default_emu_2_8.json)."""
    import json
    import os
    from oracle import cref
    from ministark_amd import GOLDILOCKS_FP
    want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "prove_phases_default_emu_2_8.json")))
    pl = backends.planner("emu")
    n_t, ncols, seed = 1 << 8, 8, 4242
    cols = [cref.random_elements(n_t, seed + c) for c in range(ncols)]
    comp, ce, nch = pipeline.fib_constraints(n_t, ncols)
    draws = pipeline.Draws(seed, ncols, nch, ce, 32, n_t * 4, pipeline.fri_num_layers(n_t * 4, 4, 8, 64))
    out = pipeline.prove_phases(pl, Matrix.from_numpy(pl, cols, GOLDILOCKS_FP), comp, draws, ce_blowup=ce)
    got = {"base_root": bytes(out["base_root"]).hex(), "composition_root": bytes(out["composition_root"]).hex(),
           "fri_roots": [bytes(r).hex() for r in out["fri_roots"]], "nonce": int(out["nonce"]),
           "remainder": [int(v) for v in out["remainder"].to_numpy()], "remainder_coeffs": [int(v) for v in out["remainder_coeffs"]]}
    assert got == want
