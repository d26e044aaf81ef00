"""Which kernels every NTT / LDE / evaluate route launches, pinned by name and count.

The parity tests compare values: a change of the host dispatch that sends a size down another (correct, slower) route passes all of
them.  Here every case runs on zero-filled columns with per-launch profiling on, and `{name: calls}` of `Planner.profile_read()` is
compared with a literal table -- no oracle, no random data.  The tables were read off the dispatch as it stood before the host code was
split into ms_ntt_plan.cpp / ms_ntt.cpp / ms_ntt252.cpp, and hold for both backends.  The profile names do not tell the limb-form kernels
(ntt2_kernels.h) from the round-1 ones (ntt_kernels.h) of a pass: one child process with MS_NTT_DEBUG=1 pins that, line by line.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import backends
from ministark_amd import (GOLDILOCKS_FP, GOLDILOCKS_FQ3, STARK252_FP, GpuFft, GpuIfft, GpuVec, Radix2EvaluationDomain)
from ministark_amd.api import _offset_words, _ptr_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FP, FQ3, F252 = GOLDILOCKS_FP, GOLDILOCKS_FQ3, STARK252_FP
WORDS = {FP: 1, FQ3: 3, F252: 4}
FFT_FIELD = {FP: FP, FQ3: FP, F252: F252}
NAME = {FP: "fp", FQ3: "fq3", F252: "f252"}


def _zeros(pl, n, field):
    return GpuVec.from_numpy(pl, np.zeros(n * WORDS[field], dtype=np.uint64), field)


def _profiled(pl, call):
    pl.profile(True)
    try:
        call()
        return {name: rec["calls"] for name, rec in pl.profile_read().items()}
    finally:
        pl.profile(False)


def transform_profile(kind, field, log_n, inverse, offset, ncols):
    pl = backends.planner(kind)
    n = 1 << log_n
    vecs = [_zeros(pl, n, field) for _ in range(ncols)]
    plan = (GpuIfft if inverse else GpuFft)(Radix2EvaluationDomain(n, offset, FFT_FIELD[field]), field, pl)
    try:
        return _profiled(pl, lambda: plan.enqueue(vecs))
    finally:
        plan.close()


def extend_profile(kind, entry, field, log_n, log_b, bit_reversed, ncols=2, offset=7):
    """`entry` = "lde" (ms_lde: evaluations on the trace domain in) or "evaluate" (ms_evaluate: coefficients in), through the C ABI itself:
    Matrix.evaluate answers a blow-up of 1 in natural order with a plain transform and never reaches ms_evaluate."""
    pl = backends.planner(kind)
    L = pl.lib
    n, N = 1 << log_n, 1 << (log_n + log_b)
    src = [_zeros(pl, n, field) for _ in range(ncols)]
    dst = [_zeros(pl, N, field) for _ in range(ncols)]
    off = _offset_words(field, offset)
    if entry == "lde":
        call = lambda: L.check(L.ms_lde(pl.handle, field, log_n, log_b, off.ctypes.data, _ptr_array(src), _ptr_array(dst), ncols, int(bit_reversed)))
    else:
        call = lambda: L.check(L.ms_evaluate(pl.handle, field, log_n, log_n + log_b, off.ctypes.data, _ptr_array(src), _ptr_array(dst), ncols, int(bit_reversed)))
    return _profiled(pl, call)


# ---- transforms: (field, log_n, inverse, offset, ncols) -> {profile name: calls} -------------------------------------------------------
# three columns where a launch packs columns (2^11: two per workgroup) or a group of columns could split (2^20: the two-stream size)
def _ncols(log_n):
    return 3 if log_n in (11, 20) else 2


_SMALL = {"ntt_small": 1}
_TINY = {"ntt_fused_tiny": 1}
_FUSED = {"ntt_fused_small": 1}
_TWO = {"ntt_pass1": 1, "ntt_pass2": 1}
_THREE = {"ntt_pass1": 1, "ntt_pass2": 1, "ntt_pass3": 1}
_FOUR = {"ntt_pass1": 1, "ntt_pass2": 1, "ntt_pass3": 1, "ntt_pass4": 1}
_LDE2 = {"lde2_pass_a": 1, "lde2_pass_b": 1}
_FP_ROUTE = {8: _SMALL, 10: _SMALL, 11: _TINY, 12: _FUSED, 14: _FUSED, 15: _TWO, 16: _TWO, 17: _THREE, 18: _LDE2, 19: _THREE, 20: _THREE}
TRANSFORMS = [((FP, log_n, inverse, offset, _ncols(log_n)), route)
              for log_n, route in _FP_ROUTE.items() for inverse in (False, True) for offset in (1, 7)]
# Fq3 columns take neither the fused nor the two-pass Fp routes
_FQ3_ROUTE = {11: _SMALL, 12: _TWO, 17: _THREE, 18: _THREE}
TRANSFORMS += [((FQ3, log_n, inverse, 7, _ncols(log_n)), route) for log_n, route in _FQ3_ROUTE.items() for inverse in (False, True)]
# the 252-bit field: one launch per column and stage group below 2^11 points (2 columns), the tiled passes from there on
_F252_ROUTE = {8: {"bit_reverse": 0, "ntt252_local": 2}, 10: {"bit_reverse": 0, "ntt252_local": 2, "ntt252_stages": 2},
               11: {"ntt252_pass1": 1, "ntt252_pass2": 1}, 12: {"ntt252_pass1": 1, "ntt252_pass2": 1}}
TRANSFORMS += [((F252, log_n, inverse, 1 if inverse else 3, 2), {k: v for k, v in route.items() if v})
               for log_n, route in _F252_ROUTE.items() for inverse in (False, True)]
# one column, on the device alone: the three-pass plan at its largest size and the four-pass plan
TRANSFORMS_HIP = [((FP, 24, False, 7, 1), _THREE), ((FP, 25, False, 1, 1), _FOUR)]


def _tid(case):
    field, log_n, inverse, offset, ncols = case
    return f"{NAME[field]}-2^{log_n}-{'inv' if inverse else 'fwd'}-off{offset}-x{ncols}"


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("case,want", TRANSFORMS, ids=[_tid(c) for c, _ in TRANSFORMS])
def test_transform_route(kind, case, want):
    got = transform_profile(kind, *case)
    print(_tid(case), got)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("case,want", TRANSFORMS_HIP, ids=[_tid(c) for c, _ in TRANSFORMS_HIP])
def test_transform_route_large_hip(case, want):
    got = transform_profile("hip", *case)
    print(_tid(case), got)
    assert got == want


# ---- ms_lde / ms_evaluate: (entry, field, log_n, log_b, bit_reversed) -> {profile name: calls} ------------------------------------------
# the inverse transform of ms_lde comes first in its rows; ms_evaluate starts from coefficients.  At blow-ups 2^0 and 2^1 the two entry
# points differ: ms_lde prunes pass 1 and fuses the bit reversal there too, ms_evaluate copies, pads, transforms and bit-reverses.
_BR = {"bit_reverse": 1}
EXTENDS = [
    # 2^10 x 4 = 2^12 points
    (("lde", FP, 10, 2, True), {**_SMALL, **_TWO}), (("lde", FP, 10, 2, False), {**_SMALL, **_TWO}),
    (("evaluate", FP, 10, 2, True), _TWO), (("evaluate", FP, 10, 2, False), _TWO),
    # 2^12 x 1
    (("lde", FP, 12, 0, True), {**_FUSED, **_TWO}), (("lde", FP, 12, 0, False), {"ntt_fused_small": 2}),
    (("evaluate", FP, 12, 0, True), {**_FUSED, **_BR}), (("evaluate", FP, 12, 0, False), _FUSED),
    # 2^12 x 2
    (("lde", FP, 12, 1, True), {**_FUSED, **_TWO}), (("lde", FP, 12, 1, False), {**_FUSED, **_TWO}),
    (("evaluate", FP, 12, 1, True), {**_FUSED, **_BR}), (("evaluate", FP, 12, 1, False), _FUSED),
    # 2^12 x 4
    (("lde", FP, 12, 2, True), {**_FUSED, **_TWO}), (("lde", FP, 12, 2, False), {**_FUSED, **_TWO}),
    (("evaluate", FP, 12, 2, True), _TWO), (("evaluate", FP, 12, 2, False), _TWO),
    # 2^12 x 32: beyond the pruned first pass
    (("lde", FP, 12, 5, True), {**_FUSED, **_THREE, **_BR}), (("lde", FP, 12, 5, False), {**_FUSED, **_THREE}),
    (("evaluate", FP, 12, 5, True), {**_THREE, **_BR}), (("evaluate", FP, 12, 5, False), _THREE),
    # 2^17 x 2: the two-pass coset LDE
    (("lde", FP, 17, 1, True), {**_THREE, **_LDE2}), (("lde", FP, 17, 1, False), {**_THREE, **_LDE2, **_BR}),
    (("evaluate", FP, 17, 1, True), _LDE2), (("evaluate", FP, 17, 1, False), {**_LDE2, **_BR}),
    # Fq3
    (("lde", FQ3, 12, 2, True), {"ntt_pass1": 2, "ntt_pass2": 2}), (("evaluate", FQ3, 12, 2, True), _TWO),
    (("lde", FQ3, 18, 1, True), {**_THREE, **_LDE2}), (("evaluate", FQ3, 18, 1, True), _LDE2),
    # the 252-bit field
    (("lde", F252, 10, 2, True), {"bit_reverse": 0, "ntt252_local": 2, "ntt252_stages": 2, "ntt252_pass1": 1, "ntt252_pass2": 1}),
    (("lde", F252, 11, 1, True), {"ntt252_pass1": 2, "ntt252_pass2": 2}),
]


def _eid(case):
    entry, field, log_n, log_b, bit_reversed = case
    return f"{entry}-{NAME[field]}-2^{log_n}-x2^{log_b}-{'bitrev' if bit_reversed else 'natural'}"


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("case,want", EXTENDS, ids=[_eid(c) for c, _ in EXTENDS])
def test_extend_route(kind, case, want):
    entry, field, log_n, log_b, bit_reversed = case
    got = extend_profile(kind, entry, field, log_n, log_b, bit_reversed, offset=3 if field == F252 else 7)
    print(_eid(case), got)
    assert got == {k: v for k, v in want.items() if v}


# ---- the kernel family of every pass (MS_NTT_DEBUG is read once per process: one child) ------------------------------------------------
_R1, _L, _LU = "round-1", "limb-form (ntt2)", "limb-form (ntt2), uniform inter-pass factor"


def _passes(log_n, V, *radix_family):
    return [f"[ms_ntt] log_n={log_n} V={V} pass {q + 1}/{len(radix_family)} radix 2^{r}: {fam} kernel" for q, (r, fam) in enumerate(radix_family)]


# the routes outside the pass loop (small, fused, two-pass at 2^18) print nothing
DEBUG_FP = {8: None, 10: None, 11: None, 12: None, 14: None, 15: [(8, _L), (7, _R1)], 16: [(8, _L), (8, _L)], 17: [(8, _LU), (1, _LU), (8, _L)], 18: None,
            19: [(8, _LU), (3, _LU), (8, _L)], 20: [(8, _LU), (4, _LU), (8, _L)]}
DEBUG_FQ3 = {11: None, 12: [(8, _R1), (4, _R1)], 17: [(8, _LU), (1, _LU), (8, _L)], 18: [(8, _LU), (2, _LU), (8, _L)]}


def _debug_want(case):
    field, log_n, inverse, offset, _ = case
    table = DEBUG_FP if field == FP else DEBUG_FQ3
    if table[log_n] is None:
        return []
    return _passes(log_n, WORDS[field], *table[log_n])          # the same in all four directions at these sizes


def test_pass_kernel_families_emu():
    cases = [c for c, _ in TRANSFORMS if c[0] in (FP, FQ3)]
    code = ("import os, sys\nsys.path.insert(0, %r)\nfrom tests import test_ntt_routes as t\n"
            "for i, (c, _) in enumerate(t.TRANSFORMS):\n"
            "    if c[0] in (t.FP, t.FQ3):\n"
            "        os.write(2, b'[case]\\n')\n"
            "        t.transform_profile('emu', c[0], c[1], c[2], c[3], 1)\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "MS_NTT_DEBUG": "1"}, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("[case]\n")[1:]
    assert len(blocks) == len(cases)
    for case, block in zip(cases, blocks):
        got = [ln for ln in block.splitlines() if ln.startswith("[ms_ntt]")]
        print(_tid(case), got)
        assert got == _debug_want(case), _tid(case)
