"""include/ministark_hip_poseidon.h -- Starknet's Poseidon over the 252-bit field -- against what binds it: the library exports every
symbol it declares, `_lib.Lib.poseidon_sigs` declares the same set, and rust/gpu/src/hip/sys_poseidon.rs is what the generator writes
and agrees with the header through test_rust_shim's independent C -> Rust type table.  No older header declares any of them."""
import ctypes
import glob
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_poseidon.h")
NAMES = ["ms_poseidon252_merkle", "ms_poseidon252_permute", "ms_poseidon252_rows", "ms_poseidon252_rows_row_major"]


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [p.strip() for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_header_library_and_ctypes_binding_agree():
    from ministark_amd import _lib, build
    assert sorted(_prototypes()) == NAMES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    others = [getattr(L, a) for a in dir(L) if a.endswith("sigs") and a != "poseidon_sigs"]
    assert sorted(L.poseidon_sigs) == NAMES and not [n for n in NAMES for o in others if n in o]
    assert all(len(L.poseidon_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    for older in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if older != HEADER:
            assert "poseidon" not in open(older).read().lower(), older
    text = open(HEADER).read()
    assert '#include "ministark_hip.h"' in text


def test_sys_poseidon_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.POSEIDON_OUT).read()
    assert text == gen_rust_sys.render_poseidon(gen_rust_sys.poseidon_prototypes())
    block = text[text.index('extern "C" {'):]
    rust = {m.group(1): [tuple(x.strip() for x in a.split(":", 1)) for a in m.group(2).split(",")]
            for m in re.finditer(r"pub fn (ms_[a-z0-9_]+)\((.*?)\)\s*->\s*c_int;", block)}
    c = _prototypes()
    assert sorted(rust) == sorted(c)
    for name, params in c.items():
        assert len(rust[name]) == len(params), name
        for cp, (rname, rtype) in zip(params, rust[name]):
            m = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", cp)
            assert rname.rstrip("_") == m.group(2) and rtype == _expect(m.group(1).strip()), (name, cp, rname, rtype)
    assert "pub mod sys_poseidon;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the wrapper that calls them passes as many arguments as the header declares
    plan = open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "plan.rs")).read()
    calls = re.findall(r"sys_poseidon::(ms_[a-z0-9_]+)\(([^;]*)\) \}\);", plan)
    assert sorted(n for n, _ in calls) == ["ms_poseidon252_merkle", "ms_poseidon252_rows"]
    for name, args in calls:
        depth, commas = 0, 0
        for ch in args:
            depth += ch in "(<"
            depth -= ch in ")>"
            commas += ch == "," and depth == 0
        assert commas + 1 == len(c[name]), name
    assert "pub fn poseidon252_commit_device" in plan
