"""include/ministark_hip_gaps.h -- select, fill clock gaps, pad -- against what binds it: the library exports the symbols it declares,
`_lib.Lib.gap_sigs` declares the same, rust/gpu/src/hip/sys_gaps.rs is what the generator writes and agrees with the header through
test_rust_shim's independent C -> Rust type table, the record layouts and enum values are the ones the Python mirror packs and the kernels
assume, and the older headers name none of it."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_gaps.h")
NAMES = ["ms_gap_fill", "ms_gap_plan"]
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h", "ministark_hip_logup.h", "ministark_hip_rpo_coin.h",
         "ministark_hip_lookup.h", "ministark_hip_sort.h")
CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
REPORT = ["active", "rows_out", "gaps", "max_gap", "unordered", "first_unordered", "saturated", "pad0"]


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
    assert sorted(L.gap_sigs) == NAMES
    assert not set(NAMES) & (set(L.sigs) | set(L.transcript_sigs) | set(L.keccak_sigs) | set(L.ext_sigs) | set(L.logup_sigs) | set(L.rpo_coin_sigs) | set(L.lookup_sigs)
                             | set(L.sort_sigs))
    assert all(len(L.gap_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    for n in NAMES:
        assert getattr(L, n).argtypes == L.gap_sigs[n][1]
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "ms_gap" not in text.lower(), older
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert '#include "ministark_hip_sort.h"' in text and "MS_EXT_ALWAYS" not in text             # the mask kinds are the extension header's, not restated
    assert "ms_sort" not in text and "ms_permute" not in text and "ms_lookup" not in text         # and it declares nothing under an older layer's names


def test_struct_sizes_and_members_agree_between_the_header_and_the_python_records():
    from ministark_amd import _lib
    for name, record, size in (("ms_gap_spec", _lib.GapSpecRecord, 32), ("ms_gap_report", _lib.GapReportRecord, 64), ("ms_gap_column", _lib.GapColumnRecord, 8)):
        want = [(member, CTYPE[ctype] * length if length else CTYPE[ctype]) for ctype, member, length in _members(name)]
        assert [(n, t) for n, t in record._fields_] == want, name
        assert ctypes.sizeof(record) == sum(ctypes.sizeof(t) for _, t in want) == size, name     # no padding the header does not spell out
    assert [m[1] for m in _members("ms_gap_report")] == REPORT
    assert [m[1:] for m in _members("ms_gap_spec")] == [("group", 3), ("ngroup", None), ("counter", None), ("mask", None), ("mask_col", None), ("pad0", None)]
    assert [m[1:] for m in _members("ms_gap_column")] == [("kind", None), ("src", None)]


def test_the_python_mirror_packs_the_records_of_the_header():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import extension
    enums = dict(gen_rust_sys.header_enums(HEADER))
    assert enums == {"MS_GAP_MAX_GROUP": extension.GAP_MAX_GROUP, "MS_GAP_MAX_COLUMNS": extension.GAP_MAX_COLUMNS,
                     "MS_GAP_COPY": extension._GAP_KIND["copy"], "MS_GAP_ZERO": extension._GAP_KIND["zero"],
                     "MS_GAP_COUNTER": extension._GAP_KIND["counter"], "MS_GAP_FLAG": extension._GAP_KIND["flag"]}
    assert (extension.GAP_MAX_GROUP, extension.GAP_MAX_COLUMNS) == (3, 128)
    assert extension.GapSpec(group=[5, 2], counter=4, mask=("zero", 6))._record() == [5, 2, 0, 2, 4, 2, 6, 0]   # group[3], ngroup, counter, mask, mask_col, pad0
    assert extension.GapSpec()._record() == [0, 0, 0, 0, -1, 0, 0, 0] and extension.GapSpec(group=[1, 2, 3], counter=0)._record()[:5] == [1, 2, 3, 3, 0]
    # the same mask words as ms_sort_key's
    assert extension.SortKey([0], mask=("zero", 6))._record()[4:6] == extension.GapSpec(mask=("zero", 6))._record()[5:7]


def test_the_kernel_constants_are_the_headers_and_the_tests():
    from tests import test_gap_rows
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    kernels = open(os.path.join(csrc, "gap_kernels.h")).read()
    m = re.search(r"static constexpr int NT = (\d+), ITEMS = (\d+), TILE = NT \* ITEMS, SCAN_ROUND = NT, OUT_ITEMS = (\d+), OUT_TILE = NT \* OUT_ITEMS, SLICE = (\d+);", kernels)
    nt, items, out_items, slice_ = (int(v) for v in m.groups())
    # the lengths the tests sweep are the kernels' edges
    assert (nt * items, nt, nt * out_items, slice_) == (test_gap_rows.T, test_gap_rows.R, test_gap_rows.U, test_gap_rows.S)
    assert re.search(r"MAXGROUP = (\d+), MAXCOLS = (\d+);", kernels).groups() == ("3", "128")
    host = open(os.path.join(csrc, "ms_gaps.cpp")).read()
    assert "static_assert(msgap::MAXGROUP == (int)MS_GAP_MAX_GROUP && msgap::MAXCOLS == (int)MS_GAP_MAX_COLUMNS" in host
    assert "sizeof(ms_gap_report) == 64 && sizeof(ms_gap_spec) == 32 && sizeof(ms_gap_column) == 8" in host
    build = __import__("ministark_amd.build", fromlist=["SOURCES"])
    assert "ms_gaps.cpp" in build.SOURCES and HEADER in build._deps()
    # the wrappers the simulator needs are plain read-modify-write there and the HIP atomics in the product: the one set of table_common.h
    common = open(os.path.join(csrc, "table_common.h")).read()
    emu, hip = common[common.index("#ifdef MS_EMU"):common.index("#else")], common[common.index("#else"):common.index("#endif")]
    for fn in ("add", "amax", "amin"):
        assert re.search(r"\b%s\(" % fn, emu) and re.search(r"\b%s\(" % fn, hip) and "using mstab::%s;" % fn in kernels, fn
    assert "atomic" not in emu and all(a in hip for a in ("atomicAdd", "atomicMax", "atomicMin"))
    # no position comes from an atomic: the kernels that write start[] past the counts and the fill name none, nor do the prefixes they call
    rest = kernels[kernels.index("__global__ void __launch_bounds__(NT) gap_scan"):]
    prefixes = common[common.index("__device__ __forceinline__ T block_exclusive"):]
    for text in (rest, prefixes):
        assert "add(&" not in text and "amax(" not in text and "amin(" not in text and "atomic" not in text
    assert "block_exclusive(" in rest and "prefix_in_rounds(" in rest and "T prefix_in_rounds(" in prefixes


def test_sys_gaps_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.GAPS_OUT).read()
    assert text == gen_rust_sys.render_gaps(gen_rust_sys.gaps_prototypes())
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
    for const in ("MS_GAP_MAX_GROUP: c_int = 3", "MS_GAP_MAX_COLUMNS: c_int = 128", "MS_GAP_COPY: c_int = 0", "MS_GAP_ZERO: c_int = 1", "MS_GAP_COUNTER: c_int = 2",
                  "MS_GAP_FLAG: c_int = 3"):
        assert "pub const " + const in text
    assert "pub struct ms_gap_spec { pub group: [i32; 3], pub ngroup: i32, pub counter: i32, pub mask: i32, pub mask_col: i32, pub pad0: i32 }" in text
    assert "pub struct ms_gap_report { " + ", ".join(f"pub {m}: u64" for m in REPORT) + " }" in text
    assert "pub struct ms_gap_column { pub kind: i32, pub src: i32 }" in text
    assert "pub mod sys_gaps;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.SORT_OUT).read() == gen_rust_sys.render_sort(gen_rust_sys.sort_prototypes())
