"""include/ministark_hip_keccak.h -- Keccak-256 / SHA3-256 commitments and proof-of-work -- against what binds it: the library exports
every symbol it declares, `_lib.Lib.keccak_sigs` declares the same set, and rust/gpu/src/hip/sys_keccak.rs is what the generator writes
and agrees with the header through test_rust_shim's independent C -> Rust type table.  Neither older header declares any of them, and
the generator still renders the two older files as they are committed."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_keccak.h")
NAMES = ["ms_keccak_merkle", "ms_keccak_pow_grind", "ms_keccak_rows", "ms_keccak_rows_row_major"]


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
    assert sorted(L.keccak_sigs) == NAMES and not set(NAMES) & (set(L.sigs) | set(L.transcript_sigs))
    assert all(len(L.keccak_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    for older in ("ministark_hip.h", "ministark_hip_transcript.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert not [n for n in NAMES if re.search(r"\b%s\s*\(" % n, text)], older
        assert "KECCAK" not in text and "SHA3" not in text, older
    text = open(HEADER).read()
    assert re.search(r"enum \{ MS_KECCAK256 = 0, MS_SHA3_256 = 1 \};", text) and re.search(r"enum \{ MS_HASH_KECCAK256 = 3, MS_HASH_SHA3_256 = 4 \};", text)
    assert '#include "ministark_hip_transcript.h"' in text


def test_sys_keccak_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.KECCAK_OUT).read()
    assert text == gen_rust_sys.render_keccak(gen_rust_sys.keccak_prototypes())
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
    for const in ("MS_KECCAK256: c_int = 0", "MS_SHA3_256: c_int = 1", "MS_HASH_KECCAK256: c_int = 3", "MS_HASH_SHA3_256: c_int = 4"):
        assert "pub const " + const in text
    assert "pub mod sys_keccak;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the two older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.TRANSCRIPT_OUT).read() == gen_rust_sys.render_transcript(gen_rust_sys.transcript_prototypes())
    # the wrapper that calls them passes as many arguments as the header declares
    plan = open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "plan.rs")).read()
    called = re.findall(r"sys_keccak::(ms_[a-z0-9_]+)\(", plan)
    assert sorted(called) == ["ms_keccak_merkle", "ms_keccak_rows"]
