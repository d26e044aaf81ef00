"""ms_fri_fold_dev -- the FRI fold whose challenge lies in device memory -- against ms_fri_fold handed the same challenge from the
host: identical words for the three fields, every folding factor, the smallest layers and one of several workgroups, alpha = 0, 1,
p - 1 and a random element, with and without a domain offset.  Plus its two refusals of overlapping output and the checked mode."""
import numpy as np
import pytest

from tests import backends
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as FP252, GpuVec, apply_drp
from ministark_amd.api import F252_P, FIELD_WORDS, GL_P, f252_to_mont_limbs, gl_to_mont

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = [pytest.param(FP, id="fp"), pytest.param(FQ3, id="fq3"), pytest.param(FP252, id="fp252")]


def mont(field, values):
    """canonical base-field integers -> Montgomery words (an Fq3 element takes three of them)"""
    if field == FP252:
        return np.concatenate([f252_to_mont_limbs(v) for v in values]).astype(np.uint64)
    return np.array([gl_to_mont(v) for v in values], dtype=np.uint64)


def random_elements(field, n, rng):
    V, p = FIELD_WORDS[field], (F252_P if field == FP252 else GL_P)
    return mont(field, [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n if field == FP252 else n * V)])


def alphas(field, rng):
    p, k = (F252_P if field == FP252 else GL_P), (3 if field == FQ3 else 1)
    return [mont(field, [0] * k), mont(field, [1] + [0] * (k - 1)), mont(field, [p - 1] * k), random_elements(field, 1, rng)]


def fold(pl, dev, field, log_n, ff, alpha, d_alpha, offset, evals, out):
    off = None if offset is None else offset.ctypes.data
    if dev:
        return pl.lib.ms_fri_fold_dev(pl.handle, field, log_n, ff, d_alpha.ptr, off, evals.ptr, out.ptr)
    return pl.lib.ms_fri_fold(pl.handle, field, log_n, ff, alpha.ctypes.data, off, evals.ptr, out.ptr)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_same_words_as_the_host_alpha_fold(kind, field):
    pl = backends.planner(kind)
    rng = np.random.default_rng(11 + field)
    offset = mont(FP252 if field == FP252 else FP, [3 if field == FP252 else 7])
    for ff in (2, 4, 8, 16):
        log_ff = ff.bit_length() - 1
        for log_n in (log_ff, log_ff + 1, log_ff + 2, log_ff + 3, 10):           # one chunk ... several workgroups (2^10 / 2 chunks)
            n = 1 << log_n
            evals = GpuVec.from_numpy(pl, random_elements(field, n, rng), field)
            want, got = GpuVec(pl, n // ff, field), GpuVec(pl, n // ff, field)
            for alpha in alphas(field, rng):
                d_alpha = GpuVec.from_numpy(pl, alpha, field)
                for off in (None, offset):
                    pl.lib.check(fold(pl, False, field, log_n, ff, alpha, None, off, evals, want))
                    pl.lib.check(fold(pl, True, field, log_n, ff, None, d_alpha, off, evals, got))
                    assert np.array_equal(got.to_numpy(), want.to_numpy()), (ff, log_n, alpha, off)
    # the mirror: a one-element GpuVec as alpha takes the device path
    a = alphas(field, rng)[3]
    assert np.array_equal(apply_drp(evals, GpuVec.from_numpy(pl, a, field), 16, 7).to_numpy(), apply_drp(evals, a, 16, 7).to_numpy())
    with pytest.raises(ValueError):
        apply_drp(evals, GpuVec.from_numpy(pl, np.concatenate([a, a]), field), 16)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_overlapping_output_is_refused_and_nothing_is_written(kind, field):
    pl = backends.planner(kind)
    rng = np.random.default_rng(3)
    V, n, ff = FIELD_WORDS[field], 64, 4
    words = random_elements(field, n + 1, rng)                      # n evaluations and one more element
    buf = GpuVec.from_numpy(pl, words, field)
    evals = GpuVec(pl, n, field, ptr=buf.ptr)
    far = GpuVec.from_numpy(pl, words[: V], field)
    for out_ptr in (buf.ptr + (n - 1) * V * 8, buf.ptr, buf.ptr - (n // ff - 1) * V * 8):          # the last / first evaluations
        rc = pl.lib.ms_fri_fold_dev(pl.handle, field, 6, ff, far.ptr, None, evals.ptr, out_ptr)
        assert rc == -1 and "d_out overlaps d_evals" in pl.lib.ms_last_error().decode()
        assert np.array_equal(buf.to_numpy(), words)
    # the output's last element is the one d_alpha points to; the evaluations it folds are elsewhere
    out = GpuVec.from_numpy(pl, words[: (n // ff) * V], field)
    rc = pl.lib.ms_fri_fold_dev(pl.handle, field, 6, ff, out.ptr + (n // ff - 1) * V * 8, None, evals.ptr, out.ptr)
    assert rc == -1 and "d_out overlaps the element at d_alpha" in pl.lib.ms_last_error().decode()
    assert np.array_equal(out.to_numpy(), words[: (n // ff) * V])
    assert pl.lib.ms_fri_fold_dev(pl.handle, field, 6, ff, None, None, evals.ptr, out.ptr) == -1


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_checked_mode_scans_the_device_alpha(kind, field):
    pl = backends.planner(kind)
    rng = np.random.default_rng(4)
    V = FIELD_WORDS[field]
    evals = GpuVec.from_numpy(pl, random_elements(field, 16, rng), field)
    out = GpuVec(pl, 8, field)
    bad = np.array([(1 << 64) - 1] * V, dtype=np.uint64)            # >= p in every field
    d_bad, d_ok = GpuVec.from_numpy(pl, bad, field), GpuVec.from_numpy(pl, random_elements(field, 1, rng), field)
    before = out.to_numpy()
    pl.checked(True)
    try:
        rc = pl.lib.ms_fri_fold_dev(pl.handle, field, 4, 2, d_bad.ptr, None, evals.ptr, out.ptr)
        msg = pl.lib.ms_last_error().decode()
        assert rc == -1 and msg.startswith("ms_fri_fold_dev: d_alpha holds an element that is not canonical") and "column 0, row 0" in msg
        assert np.array_equal(out.to_numpy(), before)
        pl.lib.check(pl.lib.ms_fri_fold_dev(pl.handle, field, 4, 2, d_ok.ptr, None, evals.ptr, out.ptr))
    finally:
        pl.checked(False)
    assert pl.lib.ms_fri_fold_dev(pl.handle, field, 4, 2, d_bad.ptr, None, evals.ptr, out.ptr) == 0      # unchecked: the caller's duty
