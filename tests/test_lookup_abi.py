"""include/ministark_hip_lookup.h -- the multiplicity column of a LogUp lookup -- against what binds it: the library exports the symbol it
declares, `_lib.Lib.lookup_sigs` declares the same, rust/gpu/src/hip/sys_lookup.rs is what the generator writes and agrees with the header
through test_rust_shim's independent C -> Rust type table, the record layouts and enum values are the ones the Python mirror packs and
the kernels assume, and the older headers name none of it."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_lookup.h")
NAMES = ["ms_lookup_multiplicities"]
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h", "ministark_hip_logup.h", "ministark_hip_rpo_coin.h")
CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    return {m.group(1): [p.strip() for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}


def _members(name):
    """[(C type, member name, array length or None)] of a typedef'd struct of the header, in order"""
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    out = []
    for m in re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text).group(1).split(";"):
        if m.strip():
            ctype, member = m.split()
            arr = re.match(r"(\w+)\[(\d+)\]$", member)
            out.append((ctype, arr.group(1), int(arr.group(2))) if arr else (ctype, member, None))
    return out


def test_header_library_and_ctypes_binding_agree():
    from ministark_amd import _lib, build
    assert sorted(_prototypes()) == NAMES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.lookup_sigs) == NAMES
    assert not set(NAMES) & (set(L.sigs) | set(L.transcript_sigs) | set(L.keccak_sigs) | set(L.ext_sigs) | set(L.logup_sigs) | set(L.rpo_coin_sigs))
    assert all(len(L.lookup_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    assert L.ms_lookup_multiplicities.argtypes == L.lookup_sigs["ms_lookup_multiplicities"][1]
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "ms_lookup" not in text.lower(), older
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert '#include "ministark_hip_ext.h"' in text and "MS_EXT_ALWAYS" not in text              # the mask kinds are the extension header's, not restated


def test_struct_sizes_and_members_agree_between_the_header_and_the_python_records():
    from ministark_amd import _lib
    for name, record in (("ms_lookup_tuple", _lib.LookupTupleRecord), ("ms_lookup_report", _lib.LookupReportRecord)):
        want = [(member, CTYPE[ctype] * length if length else CTYPE[ctype]) for ctype, member, length in _members(name)]
        assert [(n, t) for n, t in record._fields_] == want, name
        assert ctypes.sizeof(record) == sum(ctypes.sizeof(t) for _, t in want) == 32, name       # no padding the header does not spell out
    assert [m[1] for m in _members("ms_lookup_report")] == ["missing", "first_missing_row", "first_missing_set", "pad", "duplicate_table_rows"]
    assert [m[1:] for m in _members("ms_lookup_tuple")] == [("cols", 4), ("mask", None), ("mask_col", None), ("pad0", None), ("pad1", None)]


def test_the_python_mirror_packs_the_records_of_the_header():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import extension
    enums = dict(gen_rust_sys.header_enums(HEADER))
    assert enums == {"MS_LOOKUP_MAX_WIDTH": extension.LOOKUP_MAX_WIDTH, "MS_LOOKUP_MAX_SETS": extension.LOOKUP_MAX_SETS}
    assert (extension.LOOKUP_MAX_WIDTH, extension.LOOKUP_MAX_SETS) == (4, 8)
    assert extension.LookupTuple([5, 2], mask=("zero", 6))._record() == [5, 2, 0, 0, 2, 6, 0, 0]       # cols[4], mask, mask_col, pad0, pad1
    assert extension.LookupTuple([1, 2, 3, 4])._record() == [1, 2, 3, 4, 0, 0, 0, 0] and extension.LookupTuple([7], mask=("nonzero", 1))._record()[4:6] == [1, 1]
    # the same mask words as ms_ext_column's
    assert extension.ExtColumn(0, [], [], mask=("zero", 6))._record()[2:4] == extension.LookupTuple([0], mask=("zero", 6))._record()[4:6]


def test_the_kernel_constants_are_the_headers():
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    kernels = open(os.path.join(csrc, "lookup_kernels.h")).read()
    assert re.search(r"static constexpr int NT = (\d+), MAXW = (\d+), MAXSETS = (\d+);", kernels).groups() == ("256", "4", "8")
    assert "static constexpr uint32_t EMPTY = 0xFFFFFFFFu;" in kernels
    host = open(os.path.join(csrc, "ms_lookup.cpp")).read()
    assert "static_assert(mslk::MAXW == (int)MS_LOOKUP_MAX_WIDTH && mslk::MAXSETS == (int)MS_LOOKUP_MAX_SETS" in host
    build = __import__("ministark_amd.build", fromlist=["SOURCES"])
    assert "ms_lookup.cpp" in build.SOURCES and HEADER in build._deps()
    # the wrappers the simulator needs are plain read-modify-write there and the HIP atomics in the product: the one set of table_common.h
    common = open(os.path.join(csrc, "table_common.h")).read()
    emu, hip = common[common.index("#ifdef MS_EMU"):common.index("#else")], common[common.index("#else"):common.index("#endif")]
    for fn in ("cas", "amin", "add", "peek"):
        assert re.search(r"\b%s\(" % fn, emu) and re.search(r"\b%s\(" % fn, hip) and "using mstab::%s;" % fn in kernels, fn
    assert "atomic" not in emu and all(a in hip for a in ("atomicCAS", "atomicMin", "atomicAdd"))


def test_sys_lookup_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.LOOKUP_OUT).read()
    assert text == gen_rust_sys.render_lookup(gen_rust_sys.lookup_prototypes())
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
    for const in ("MS_LOOKUP_MAX_WIDTH: c_int = 4", "MS_LOOKUP_MAX_SETS: c_int = 8"):
        assert "pub const " + const in text
    assert "pub struct ms_lookup_tuple { pub cols: [i32; 4], pub mask: i32, pub mask_col: i32, pub pad0: i32, pub pad1: i32 }" in text
    assert "pub struct ms_lookup_report { pub missing: u64, pub first_missing_row: u64, pub first_missing_set: u32, pub pad: u32, pub duplicate_table_rows: u64 }" in text
    assert "pub mod sys_lookup;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.EXT_OUT).read() == gen_rust_sys.render_ext(gen_rust_sys.ext_prototypes())
    assert open(gen_rust_sys.LOGUP_OUT).read() == gen_rust_sys.render_logup(gen_rust_sys.logup_prototypes())
    assert open(gen_rust_sys.RPO_COIN_OUT).read() == gen_rust_sys.render_rpo_coin(gen_rust_sys.rpo_coin_prototypes())
