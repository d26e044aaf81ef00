"""include/ministark_hip_ext.h -- the extension columns between the two trace commitments -- against what binds it: the library exports the
symbol it declares, `_lib.Lib.ext_sigs` declares the same, rust/gpu/src/hip/sys_ext.rs is what the generator writes and agrees with the
header through test_rust_shim's independent C -> Rust type table, the record layouts are the ones the Python mirror packs, and the older
headers and generated files are untouched by it."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_ext.h")
NAMES = ["ms_build_extension_columns"]


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
    assert sorted(L.ext_sigs) == NAMES and not set(NAMES) & (set(L.sigs) | set(L.transcript_sigs) | set(L.keccak_sigs))
    assert all(len(L.ext_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    for older in ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "ms_build_extension_columns" not in text and "MS_EXT_" not in text, older
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    # the records the Python mirror packs as rows of int32: 4 words per term, 8 per column -- the members in order, whatever the layout of the text
    members = lambda name: [tuple(m.split()) for m in re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text).group(1).split(";") if m.strip()]
    assert members("ms_ext_term") == [("int32_t", "col"), ("int32_t", "off"), ("int32_t", "chal"), ("int32_t", "sign")]
    assert members("ms_ext_column") == [("int32_t", "init"), ("int32_t", "init_chal"), ("int32_t", "mask"), ("int32_t", "mask_col"), ("int32_t", "inclusive"),
                                        ("uint32_t", "na"), ("uint32_t", "nb"), ("uint32_t", "pad")]
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import extension
    enums = dict(gen_rust_sys.header_enums(HEADER))
    assert (enums["MS_EXT_MAX_TERMS"], enums["MS_EXT_MAX_COLUMNS"], enums["MS_EXT_NONE"]) == (extension.MAX_TERMS, extension.MAX_COLUMNS, extension.NONE)
    assert (enums["MS_EXT_INIT_ZERO"], enums["MS_EXT_INIT_ONE"], enums["MS_EXT_INIT_CHALLENGE"]) == (0, 1, 2)
    assert (enums["MS_EXT_ALWAYS"], enums["MS_EXT_IF_NONZERO"], enums["MS_EXT_IF_ZERO"]) == (0, extension._MASK["nonzero"], extension._MASK["zero"])
    # the rows a workgroup scans, which the length sweep of test_extension_columns.py is built around: msscan::NT lanes x msext::PER rows
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    nt = int(re.search(r"static constexpr int NT = (\d+);", open(os.path.join(csrc, "scan_kernels.h")).read()).group(1))
    per = int(re.search(r"static constexpr int PER = (\d+);", open(os.path.join(csrc, "ext_kernels.h")).read()).group(1))
    assert "static constexpr int ROWS = NT * PER;" in open(os.path.join(csrc, "ext_kernels.h")).read()
    assert extension.ROWS_PER_WORKGROUP == nt * per


def test_sys_ext_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.EXT_OUT).read()
    assert text == gen_rust_sys.render_ext(gen_rust_sys.ext_prototypes())
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
    for const in ("MS_EXT_MAX_TERMS: c_int = 8", "MS_EXT_MAX_COLUMNS: c_int = 32", "MS_EXT_NONE: c_int = -1", "MS_EXT_INIT_CHALLENGE: c_int = 2", "MS_EXT_IF_ZERO: c_int = 2"):
        assert "pub const " + const in text
    assert "pub struct ms_ext_term { pub col: i32, pub off: i32, pub chal: i32, pub sign: i32 }" in text
    assert "pub mod sys_ext;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the three older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.TRANSCRIPT_OUT).read() == gen_rust_sys.render_transcript(gen_rust_sys.transcript_prototypes())
    assert open(gen_rust_sys.KECCAK_OUT).read() == gen_rust_sys.render_keccak(gen_rust_sys.keccak_prototypes())
