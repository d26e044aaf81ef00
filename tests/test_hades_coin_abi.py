"""include/ministark_hip_hades_coin.h -- the Poseidon public coin of the 252-bit field -- against what binds it, with the method of
tests/test_poseidon_abi.py: the library exports every symbol the header declares, `_lib.Lib.hades_coin_sigs` declares the same set with
the argument types of the RPO-256 coin's namesakes, and rust/gpu/src/hip/sys_hades_coin.rs is what the generator writes and agrees with
the header through test_rust_shim's independent C -> Rust type table.  No other header declares any of them, and this one keeps to the
permutation's name: tests/test_poseidon_abi.py reserves the hash's name for include/ministark_hip_poseidon.h."""
import ctypes
import glob
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_hades_coin.h")
NAMES = sorted("ms_hades_coin_" + n for n in ("create", "destroy", "read", "write", "reseed_digest", "reseed_int", "reseed_elements",
                                               "reseed_elements_host", "draw", "draw_queries", "pow_grind"))


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    return {m.group(1): [p.strip() for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}


def test_header_library_and_ctypes_binding_agree():
    from ministark_amd import _lib, build
    protos = _prototypes()
    assert sorted(protos) == NAMES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.hades_coin_sigs) == NAMES
    others = [getattr(L, a) for a in dir(L) if a.endswith("sigs") and a != "hades_coin_sigs"]
    assert len(others) >= 11 and not [n for n in NAMES for o in others if n in o]
    assert sorted(L.poseidon_sigs) == ["ms_poseidon252_merkle", "ms_poseidon252_permute", "ms_poseidon252_rows", "ms_poseidon252_rows_row_major"]
    for name, params in protos.items():
        assert len(L.hades_coin_sigs[name][1]) == len(params), name
        assert getattr(L, name).argtypes == L.hades_coin_sigs[name][1]
        assert L.hades_coin_sigs[name] == L.rpo_coin_sigs[name.replace("ms_hades_coin_", "ms_rpo_coin_")], name    # each the twin of its namesake
    text = open(HEADER).read()
    assert "poseidon" not in text.lower()
    assert "the Hades permutation (t = 3, x^3, 8 + 83 rounds) of the library's algebraic 252-bit commitment" in " ".join(text.replace(" * ", " ").split())
    for other in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if other != HEADER:
            assert "hades_coin" not in re.sub(r"/\*.*?\*/", "", open(other).read(), flags=re.S).lower(), other
    code = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert '#include "ministark_hip_transcript.h"' in code and code.count("#include") == 1
    body = re.search(r"typedef struct ms_hades_coin_state \{(.*?)\} ms_hades_coin_state;", code).group(1)
    assert [tuple(m.split()) for m in body.split(";") if m.strip()] == [("uint64_t", "digest[4]"), ("uint64_t", "n_draws"), ("uint32_t", "pad[4]")]
    assert ctypes.sizeof(_lib.HadesCoinState) == 56 and ctypes.alignment(_lib.HadesCoinState) == 8
    assert [(n, ctypes.sizeof(t)) for n, t in _lib.HadesCoinState._fields_] == [("digest", 32), ("n_draws", 8), ("pad", 16)]
    assert _lib.HadesCoinState.n_draws.offset == 32 and _lib.HadesCoinState.pad.offset == 40
    kernels = open(os.path.join(ROOT, "ministark_amd", "csrc", "hades_coin_kernels.h")).read()
    assert "static_assert(sizeof(State) == 56" in kernels
    assert "ms_hades_coin.cpp" in build.SOURCES and "ms_poseidon.cpp" in build.SOURCES


def test_sys_hades_coin_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.HADES_COIN_OUT).read()
    assert text == gen_rust_sys.render_hades_coin(gen_rust_sys.hades_coin_prototypes())
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
    assert "pub struct ms_hades_coin_state { pub digest: [u64; 4], pub n_draws: u64, pub pad: [u32; 4] }" in text
    assert "pub mod sys_hades_coin;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the older files still come out of the generator as committed
    assert open(gen_rust_sys.RPO_COIN_OUT).read() == gen_rust_sys.render_rpo_coin(gen_rust_sys.rpo_coin_prototypes())
    assert open(gen_rust_sys.POSEIDON_OUT).read() == gen_rust_sys.render_poseidon(gen_rust_sys.poseidon_prototypes())
    assert open(gen_rust_sys.TRANSCRIPT_OUT).read() == gen_rust_sys.render_transcript(gen_rust_sys.transcript_prototypes())
