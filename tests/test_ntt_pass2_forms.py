"""Pass 2 of the three-pass NTT plans after its change of form: the per-lane factor on the loads as ONE plain word
(glimb::mul_to_limbs, signed limbs into the network), read ready-made from the plan's lq table, and the wave-uniform
factor after the second network from twu4 in wave order ([U][a'][d], four factors per 128-byte line).

The radix-256 middle pass (ntt2_mid_pass<.., LOADQ, PERM>) exists only at 2^24 points (middle radix = n / 2^16), so that is
the smallest shape that can go wrong: all four plans on the device, every output word against the oracle, and the forward
coset transform once under the CPU simulator (about ten seconds: the one slow case of this file).
ntt2_mid_pass_r (middle radix 32 .. 128, 2^21 .. 2^23 points) took the one-word product too: forward and inverse coset on the
device at 2^21 and 2^23 and under the simulator at 2^21 and 2^22; 2^17 and 2^20 (ntt2_small_mid_pass, which kept the three-copy
product) ride along on the device as the unchanged neighbours.
"""
import functools

import numpy as np
import pytest

from oracle import cref
from tests import backends
from ministark_amd import GOLDILOCKS_FP, GpuFft, GpuIfft, GpuVec, Radix2EvaluationDomain

PLANS = [pytest.param(False, 7, id="forward-coset"), pytest.param(False, 1, id="forward-subgroup"),
         pytest.param(True, 7, id="inverse-coset"), pytest.param(True, 1, id="inverse-subgroup")]


@functools.lru_cache(maxsize=None)
def _column(log_n, kind="random"):
    n = 1 << log_n
    if kind == "zero":
        c = np.zeros(n, dtype=np.uint64)
    elif kind == "pm1":
        c = np.full(n, cref.GL_P - 1, dtype=np.uint64)
    else:
        c = cref.random_elements(n, 5150 + log_n)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(log_n, inverse, offset, kind="random"):
    w = cref.ntt(np.array(_column(log_n, kind)), log_n, 1, inverse, offset)
    w.setflags(write=False)
    return w


def _check(got, want, what):
    bad = np.nonzero(want != got)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:8]}"


def _one_column(kind, log_n, inverse, offset):
    pl = backends.planner(kind)
    v = GpuVec.from_numpy(pl, np.array(_column(log_n)), GOLDILOCKS_FP)
    plan = (GpuIfft if inverse else GpuFft)(Radix2EvaluationDomain(1 << log_n, offset), GOLDILOCKS_FP, pl)
    plan.encode(v)
    plan.execute()
    plan.close()
    _check(v.to_numpy(), _want(log_n, inverse, offset), f"2^{log_n} inverse={inverse} offset={offset}")


@pytest.mark.gpu
@pytest.mark.parametrize("inverse,offset", PLANS)
def test_radix256_middle_pass_all_plans_hip(inverse, offset):
    _one_column("hip", 24, inverse, offset)


@pytest.mark.gpu
def test_radix256_middle_pass_three_columns_hip():
    # one launch, three columns: random, all zero, all p - 1 (the largest canonical word in every product on the loads)
    pl = backends.planner("hip")
    kinds = ("random", "zero", "pm1")
    vecs = [GpuVec.from_numpy(pl, np.array(_column(24, k)), GOLDILOCKS_FP) for k in kinds]
    plan = GpuFft(Radix2EvaluationDomain(1 << 24, 7), GOLDILOCKS_FP, pl)
    plan.enqueue(vecs)
    for k, v in zip(kinds, vecs):
        _check(v.to_numpy(), _want(24, False, 7, k), f"column {k}")
    plan.close()


@pytest.mark.gpu
def test_radix256_middle_pass_out_of_place_hip():
    # ms_ntt_enqueue_to: the source stays, pass 2 still runs in place on the scratch column
    pl = backends.planner("hip")
    src = GpuVec.from_numpy(pl, np.array(_column(24)), GOLDILOCKS_FP)
    dst = GpuVec(pl, 1 << 24, GOLDILOCKS_FP)
    plan = GpuFft(Radix2EvaluationDomain(1 << 24, 7), GOLDILOCKS_FP, pl)
    plan.enqueue_to([src], [dst])
    _check(dst.to_numpy(), _want(24, False, 7), "destination")
    _check(src.to_numpy(), _column(24), "source")
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [17, 20, 21, 23])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward-coset", "inverse-coset"])
def test_smaller_middle_radices_hip(log_n, inverse):
    _one_column("hip", log_n, inverse, 7)


@pytest.mark.parametrize("log_n", [21, 22])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward-coset", "inverse-coset"])
def test_smaller_middle_radices_emu(log_n, inverse):
    _one_column("emu", log_n, inverse, 7)


def test_radix256_middle_pass_forward_coset_emu():
    _one_column("emu", 24, False, 7)
