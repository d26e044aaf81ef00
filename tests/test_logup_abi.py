"""include/ministark_hip_logup.h -- the LogUp lookup columns -- against what binds it: the library exports the symbol it declares,
`_lib.Lib.logup_sigs` declares the same, rust/gpu/src/hip/sys_logup.rs is what the generator writes and agrees with the header through
test_rust_shim's independent C -> Rust type table, the record layouts and enum values are the ones the Python mirror packs, the rows per
workgroup and per lane the length sweep of test_logup_columns.py is built around are the kernels', and the older headers name none of it."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_logup.h")
NAMES = ["ms_build_logup_columns"]
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h")


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    return {m.group(1): [p.strip() for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}


def test_header_library_and_ctypes_binding_agree():
    from ministark_amd import _lib, build
    assert sorted(_prototypes()) == NAMES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.logup_sigs) == NAMES
    assert not set(NAMES) & (set(L.sigs) | set(L.transcript_sigs) | set(L.keccak_sigs) | set(L.ext_sigs))
    assert all(len(L.logup_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    assert L.ms_build_logup_columns.argtypes == L.logup_sigs["ms_build_logup_columns"][1]
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "logup" not in text.lower(), older
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert '#include "ministark_hip_ext.h"' in text and "ms_ext_term" not in text          # the terms are the extension header's, not restated
    # the records the Python mirror packs as rows of 32-bit words: 8 per column, 2 per fraction -- the members in order
    members = lambda name: [tuple(m.split()) for m in re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text).group(1).split(";") if m.strip()]
    assert members("ms_logup_column") == [("int32_t", "init"), ("int32_t", "init_chal"), ("int32_t", "mask"), ("int32_t", "mask_col"), ("int32_t", "inclusive"),
                                          ("uint32_t", "nf"), ("uint32_t", "pad0"), ("uint32_t", "pad1")]
    assert members("ms_logup_fraction") == [("uint32_t", "nn"), ("uint32_t", "nd")]


def test_the_python_mirror_packs_the_records_of_the_header():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import extension
    enums = dict(gen_rust_sys.header_enums(HEADER))
    assert enums == {"MS_LOGUP_MAX_FRACTIONS": extension.LOGUP_MAX_FRACTIONS, "MS_LOGUP_MAX_COLUMNS": extension.LOGUP_MAX_COLUMNS}
    assert (extension.LOGUP_MAX_FRACTIONS, extension.LOGUP_MAX_COLUMNS) == (4, 32)
    num, den = [(+1, None, 4, 7)], [(+1, 0, None), (-1, 1, 3, -2)]
    c = extension.LogUpColumn(("challenge", 3), [(num, den), ([], den[:1])], mask=("zero", 6), inclusive=True)
    assert c._record() == [2, 3, 2, 6, 1, 2, 0, 0]                            # init, init_chal, mask, mask_col, inclusive, nf, pad0, pad1
    assert c._fractions() == [[1, 2], [0, 1]]                                  # nn, nd
    assert c._terms() == [[4, 7, -1, 1], [-1, 0, 0, 1], [3, -2, 1, -1], [-1, 0, 0, 1]]      # col, off, chal, sign: numerator, then denominator
    assert extension.LogUpColumn(0, [])._record() == [0, 0, 0, 0, 0, 0, 0, 0] and extension.LogUpColumn(1, [], mask=("nonzero", 2))._record()[:4] == [1, 0, 1, 2]
    # the same head as ms_ext_column's
    assert extension.ExtColumn(("challenge", 3), [], [], mask=("zero", 6), inclusive=True)._record()[:5] == c._record()[:5]


def test_the_kernel_constants_are_the_ones_the_tests_are_built_around():
    from ministark_amd import extension
    from tests import test_logup_columns
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    logup = open(os.path.join(csrc, "logup_kernels.h")).read()
    nt = int(re.search(r"static constexpr int NT = (\d+);", open(os.path.join(csrc, "scan_kernels.h")).read()).group(1))
    per = int(re.search(r"static constexpr int PER = (\d+);", open(os.path.join(csrc, "ext_kernels.h")).read()).group(1))
    assert "using msext::PER;" in logup and "using msext::ROWS;" in logup and "using msscan::NT;" in logup      # one set of constants for both builders
    assert test_logup_columns.PER == per and test_logup_columns.B == extension.ROWS_PER_WORKGROUP == nt * per
    assert re.search(r"static constexpr int MAXFRAC = (\d+), MAXCOLS = (\d+);", logup).groups() == ("4", "32")
    assert "ms_logup.cpp" in __import__("ministark_amd.build", fromlist=["SOURCES"]).SOURCES


def test_sys_logup_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.LOGUP_OUT).read()
    assert text == gen_rust_sys.render_logup(gen_rust_sys.logup_prototypes())
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
    for const in ("MS_LOGUP_MAX_FRACTIONS: c_int = 4", "MS_LOGUP_MAX_COLUMNS: c_int = 32"):
        assert "pub const " + const in text
    assert "pub struct ms_logup_column { pub init: i32, pub init_chal: i32, pub mask: i32, pub mask_col: i32, pub inclusive: i32, pub nf: u32, pub pad0: u32, pub pad1: u32 }" in text
    assert "pub struct ms_logup_fraction { pub nn: u32, pub nd: u32 }" in text
    assert "pub mod sys_logup;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the four older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.TRANSCRIPT_OUT).read() == gen_rust_sys.render_transcript(gen_rust_sys.transcript_prototypes())
    assert open(gen_rust_sys.KECCAK_OUT).read() == gen_rust_sys.render_keccak(gen_rust_sys.keccak_prototypes())
    assert open(gen_rust_sys.EXT_OUT).read() == gen_rust_sys.render_ext(gen_rust_sys.ext_prototypes())
