"""The two places where validate_constraints splits its work, against the checked model of tests/test_validate_constraints.py:
more than 64 constraints in one program (ms_validate_constraints runs one counting launch per 64 constraints, csrc/ms_validate.cpp),
and constraints whose one program would need more registers than the interpreter has (several programs, ministark_amd/debug.py _groups)."""
import pytest

from tests import backends
from tests.test_validate_constraints import BACKENDS, failures_of, gl_matrix, model
from ministark_amd import debug
from ministark_amd import expr as E


@pytest.mark.parametrize("kind", BACKENDS)
def test_more_than_64_constraints_in_one_program(kind):
    pl = backends.planner(kind)
    n = 1 << 5
    a, z = E.Trace(0), E.Trace(1)
    # constraint k divides by z - (k mod 7): it fails where z == k mod 7 and a != 0, on rows that differ from one constraint to the next;
    # a few constraints on either side of index 64 hold everywhere
    cons = [a * E.Constant(k + 1) / (z - E.Constant(k % 7)) if k not in (3, 63, 64, 65, 130) else a - a for k in range(140)]
    cols = [[(r * 5 + 1) % 4 for r in range(n)], [r % 9 for r in range(n)]]
    prog = debug.compile_constraints(cons, 2, False)
    assert sum(1 for ins in prog.instrs if ins[0] == E.OP_STORE_P) == 140
    assert len(debug._groups(cons, 2, False, debug.GOLDILOCKS_FP)) == 1      # one program, three counting launches
    want = failures_of(model(cons, n, cols, [], [], [], False))
    assert {c for c, _, _ in want} & set(range(64)) and {c for c, _, _ in want} & set(range(64, 128)) and {c for c, _, _ in want} & set(range(128, 140))
    r = debug.validate_constraints(cons, [], [], gl_matrix(pl, cols), raise_on_failure=False)
    assert r.failures == want


@pytest.mark.parametrize("kind", BACKENDS)
def test_constraints_split_into_several_programs(kind):
    pl = backends.planner(kind)
    n = 1 << 4
    a, z = E.Trace(0), E.Trace(1)
    terms = [a ** (k + 1) / (z - E.Constant(k % 3)) for k in range(300)]

    def balanced_sum(ts):                             # a few registers on its own
        return ts[0] if len(ts) == 1 else balanced_sum(ts[:len(ts) // 2]) + balanced_sum(ts[len(ts) // 2:])
    first, second = balanced_sum(terms), balanced_sum(terms[::-1])
    # the 300 quotients stay live from the first constraint until the second reads them: one program would need > 256 registers
    cons = [a - a, first, second, z * E.Constant(0)]
    with pytest.raises(ValueError, match="registers"):
        debug.compile_constraints(cons, 2, False)
    groups = debug._groups(cons, 2, False, debug.GOLDILOCKS_FP)
    assert len(groups) >= 2 and [lo for lo, _ in groups] == sorted(lo for lo, _ in groups)
    cols = [[(r + 1) % 3 for r in range(n)], [(r * 7) % 5 for r in range(n)]]
    want = failures_of(model(cons, n, cols, [], [], [], False))
    assert [c for c, _, _ in want] == [1, 2]
    r = debug.validate_constraints(cons, [], [], gl_matrix(pl, cols), raise_on_failure=False)
    assert r.failures == want
