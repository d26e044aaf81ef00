"""include/ministark_hip_join.h -- rows joined against a table -- against what binds it: the library exports the symbol it declares,
`_lib.Lib.join_sigs` declares the same, rust/gpu/src/hip/sys_join.rs is what the generator writes and agrees with the header through
test_rust_shim's independent C -> Rust type table, the record layout and enum values are the ones the Python mirror packs and the kernels
assume, and the older headers name none of it."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_join.h")
NAMES = ["ms_join_rows"]
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h", "ministark_hip_logup.h", "ministark_hip_rpo_coin.h",
         "ministark_hip_lookup.h", "ministark_hip_sort.h", "ministark_hip_gaps.h")
CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
MEMBERS = ["matched", "missing", "first_missing_row", "first_missing_set", "pad", "duplicate_table_rows", "table_active"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototypes():
    src = re.sub(r"^\s*#.*$", "", _code(), flags=re.M)
    return {m.group(1): [p.strip() for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}


def _members(name):
    """[(C type, member name)] of a typedef'd struct of the header, in order"""
    text = " ".join(_code().split())
    return [tuple(m.split()) for m in re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text).group(1).split(";") if m.strip()]


def test_header_library_and_ctypes_binding_agree():
    from ministark_amd import _lib, build
    assert sorted(_prototypes()) == NAMES                                       # exactly one prototype
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.join_sigs) == NAMES
    others = (L.sigs, L.transcript_sigs, L.keccak_sigs, L.ext_sigs, L.logup_sigs, L.rpo_coin_sigs, L.lookup_sigs, L.sort_sigs, L.gap_sigs)
    assert not any(set(NAMES) & set(o) for o in others)
    assert all(len(L.join_sigs[n][1]) == len(params) for n, params in _prototypes().items()) and len(L.join_sigs["ms_join_rows"][1]) == 14
    assert L.ms_join_rows.argtypes == L.join_sigs["ms_join_rows"][1]
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "ms_join" not in text.lower(), older
    text = " ".join(_code().split())
    assert '#include "ministark_hip_ext.h"' in text and '#include "ministark_hip_lookup.h"' in text
    assert "MS_EXT_ALWAYS" not in text and "ms_lookup_tuple" not in text        # the mask kinds and the key record are the other headers', not restated


def test_the_report_record_is_the_headers():
    from ministark_amd import _lib
    want = [(member, CTYPE[ctype]) for ctype, member in _members("ms_join_report")]
    assert [(n, t) for n, t in _lib.JoinReportRecord._fields_] == want
    assert ctypes.sizeof(_lib.JoinReportRecord) == sum(ctypes.sizeof(t) for _, t in want) == 48        # no padding the header does not spell out
    assert [m for _, m in _members("ms_join_report")] == MEMBERS


def test_the_python_constants_are_the_headers():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import extension
    assert dict(gen_rust_sys.header_enums(HEADER)) == {"MS_JOIN_MAX_WIDTH": extension.JOIN_MAX_WIDTH, "MS_JOIN_MAX_SETS": extension.JOIN_MAX_SETS}
    assert (extension.JOIN_MAX_WIDTH, extension.JOIN_MAX_SETS) == (extension.LOOKUP_MAX_WIDTH, extension.LOOKUP_MAX_SETS) == (4, 8)
    none = re.search(r"^#define MS_JOIN_NONE (0x[0-9A-Fa-f]+)u$", _code(), flags=re.M)
    assert none and int(none.group(1), 16) == extension.JOIN_NONE == 0xFFFFFFFF


def test_the_kernels_are_the_lookup_layers_build_and_a_probe_of_their_own():
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    kernels = open(os.path.join(csrc, "join_kernels.h")).read()
    assert '#include "lookup_kernels.h"' in kernels and "lookup_build" not in re.sub(r"//.*", "", kernels)      # reused, not restated
    assert "static constexpr uint32_t NONE = 0xFFFFFFFFu;" in kernels
    for fn in ("add", "amin", "block_totals"):
        assert "using mstab::%s;" % fn in kernels
    assert "void block_totals(" not in kernels and "mstab::FirstRow" in kernels  # the workgroup reduction and the first-row decode are table_common.h's
    assert "atomic" not in re.sub(r"//.*", "", kernels)                         # every atomic goes through table_common.h, which the simulator makes exact
    host = open(os.path.join(csrc, "ms_join.cpp")).read()
    assert "static_assert(mslk::MAXW == (int)MS_JOIN_MAX_WIDTH && mslk::MAXSETS == (int)MS_JOIN_MAX_SETS" in host
    assert "sizeof(ms_join_report) == 48" in host and "mslk::lookup_build<V>" in host
    build = __import__("ministark_amd.build", fromlist=["SOURCES"])
    assert "ms_join.cpp" in build.SOURCES and HEADER in build._deps()


def test_sys_join_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.JOIN_OUT).read()
    assert text == gen_rust_sys.render_join(gen_rust_sys.join_prototypes())
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
    for const in ("MS_JOIN_MAX_WIDTH: c_int = 4", "MS_JOIN_MAX_SETS: c_int = 8", "MS_JOIN_NONE: u32 = 0xFFFFFFFF"):
        assert "pub const " + const in text
    assert ("pub struct ms_join_report { pub matched: u64, pub missing: u64, pub first_missing_row: u64, pub first_missing_set: u32, pub pad: u32, "
            "pub duplicate_table_rows: u64, pub table_active: u64 }") in text
    assert "pub mod sys_join;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.EXT_OUT).read() == gen_rust_sys.render_ext(gen_rust_sys.ext_prototypes())
    assert open(gen_rust_sys.LOGUP_OUT).read() == gen_rust_sys.render_logup(gen_rust_sys.logup_prototypes())
    assert open(gen_rust_sys.RPO_COIN_OUT).read() == gen_rust_sys.render_rpo_coin(gen_rust_sys.rpo_coin_prototypes())
    assert open(gen_rust_sys.LOOKUP_OUT).read() == gen_rust_sys.render_lookup(gen_rust_sys.lookup_prototypes())
    assert open(gen_rust_sys.SORT_OUT).read() == gen_rust_sys.render_sort(gen_rust_sys.sort_prototypes())
    assert open(gen_rust_sys.GAPS_OUT).read() == gen_rust_sys.render_gaps(gen_rust_sys.gaps_prototypes())
