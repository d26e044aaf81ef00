"""compile_expr's programs are unchanged by the multi-root lowering it now shares with compile_constraints (ministark_amd/expr.py `lower`):
tests/golden/compiled_programs.json holds the programs of the fib, additive and mixed compositions as compile_expr produced them before."""
import json
import os

import pytest

from ministark_amd import STARK252_FP, pipeline
from ministark_amd import expr as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "compiled_programs.json")))


def _dump(p):
    return {"instrs": [list(map(int, i)) for i in p.instrs], "consts": [int(c) for c in p.consts], "max_p": p.max_p, "max_q": p.max_q,
            "out_field": p.out_field, "challenge_slots": sorted([int(k), int(v)] for k, v in p.challenge_slots.items()),
            "hint_slots": sorted([int(k), int(v)] for k, v in p.hint_slots.items()), "periodic": [[list(c), iv] for c, iv in p.periodic]}


CASES = {
    "fib_2^10": lambda: E.compile_expr(pipeline.fib_constraints(1 << 10)[0], 8, False),
    "fib252_2^8": lambda: E.compile_expr(pipeline.fib_constraints(1 << 8, field=STARK252_FP)[0], 8, False, STARK252_FP),
    "additive_2^10": lambda: E.compile_expr(pipeline.additive_constraints(1 << 10)[0], 8, False),
    "additive_2^10_ext": lambda: E.compile_expr(pipeline.additive_constraints(1 << 10)[0], 8, True),
    "mixed": lambda: E.compile_expr(pipeline.mixed_air_constraints()[0], 17, True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_compile_expr_output_is_unchanged(name):
    assert _dump(CASES[name]()) == GOLDEN[name]
