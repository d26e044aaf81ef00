"""include/ministark_hip_transcript.h -- the public coin and the device-alpha fold -- against what binds it: the library exports every
symbol it declares, `_lib.Lib.transcript_sigs` declares the same set, and rust/gpu/src/hip/sys_transcript.rs is what the generator
writes and agrees with the header through test_rust_shim's independent C -> Rust type table.  ministark_hip.h declares none of them."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_transcript.h")
NAMES = ["ms_coin_create", "ms_coin_destroy", "ms_coin_draw", "ms_coin_draw_queries", "ms_coin_pow_grind", "ms_coin_read", "ms_coin_reseed_digest",
         "ms_coin_reseed_elements", "ms_coin_reseed_elements_host", "ms_coin_reseed_int", "ms_coin_write", "ms_fri_fold_dev"]


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
    assert sorted(L.transcript_sigs) == NAMES and not set(NAMES) & set(L.sigs)
    assert all(len(L.transcript_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ministark_hip.h")).read(), flags=re.S)
    assert not [n for n in NAMES if re.search(r"\b%s\s*\(" % n, main)]
    assert ctypes.sizeof(_lib.CoinState) == 80


def test_sys_transcript_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.TRANSCRIPT_OUT).read()
    assert text == gen_rust_sys.render_transcript(gen_rust_sys.transcript_prototypes())
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
    assert "pub mod sys_transcript;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
