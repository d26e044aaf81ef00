"""include/ministark_hip_blake3.h -- BLAKE3 commitments and proof-of-work -- against what binds it: the library exports every symbol it
declares, `_lib.Lib.blake3_sigs` declares the same set, and rust/gpu/src/hip/sys_blake3.rs is what the generator writes and agrees with
the header through test_rust_shim's independent C -> Rust type table.  No older header declares any of them."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_blake3.h")
NAMES = ["ms_blake3_merkle", "ms_blake3_pow_grind", "ms_blake3_rows", "ms_blake3_rows_row_major"]


def _prototypes(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
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
    others = [getattr(L, a) for a in dir(L) if a.endswith("sigs") and a != "blake3_sigs"]
    assert sorted(L.blake3_sigs) == NAMES and not [n for n in NAMES for o in others if n in o]
    # each entry point is the twin of its ms_blake2s_* namesake: the same parameters, in the same order
    twins = _prototypes(os.path.join(ROOT, "include", "ministark_hip.h"))
    for n, params in _prototypes().items():
        assert len(L.blake3_sigs[n][1]) == len(params)
        assert params == twins[n.replace("blake3", "blake2s")] and L.blake3_sigs[n] == L.sigs[n.replace("blake3", "blake2s")], n
    for older in os.listdir(os.path.join(ROOT, "include")):
        if older != "ministark_hip_blake3.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
            assert "blake3" not in text.lower(), older
    text = open(HEADER).read()
    assert re.search(r"enum \{ MS_HASH_BLAKE3 = 6 \};", text) and '#include "ministark_hip_transcript.h"' in text
    assert "ministark_hip_blake3.h" in open(os.path.join(ROOT, "ministark_amd", "build.py")).read() and "ms_blake3.cpp" in build.SOURCES


def test_sys_blake3_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.BLAKE3_OUT).read()
    assert text == gen_rust_sys.render_blake3(gen_rust_sys.blake3_prototypes())
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
    assert "pub const MS_HASH_BLAKE3: c_int = 6;" in text
    assert "pub mod sys_blake3;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the wrapper that calls them passes as many arguments as the header declares
    plan = open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "plan.rs")).read()
    assert sorted(re.findall(r"sys_blake3::(ms_[a-z0-9_]+)\(", plan)) == ["ms_blake3_merkle", "ms_blake3_rows"]
    for call in re.findall(r"sys_blake3::(ms_[a-z0-9_]+)\((.*?)\) \}\);", plan):
        assert len(re.sub(r"\([^()]*\)", "", call[1]).split(",")) == len(c[call[0]]), call[0]
