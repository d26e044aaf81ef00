"""include/ministark_hip_range.h -- range-check columns -- against what binds it: the library exports the symbols it declares,
`_lib.Lib.range_sigs` declares the same, rust/gpu/src/hip/sys_range.rs is what the generator writes and agrees with the header through
test_rust_shim's independent C -> Rust type table, the record layouts and enum values are the ones the Python mirror packs and the kernels
assume, and the older headers name none of it."""
import ctypes
import os
import re
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_range.h")
NAMES = ["ms_limb_decompose", "ms_range_multiplicities"]
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h", "ministark_hip_logup.h", "ministark_hip_rpo_coin.h",
         "ministark_hip_lookup.h", "ministark_hip_sort.h", "ministark_hip_gaps.h", "ministark_hip_join.h", "ministark_hip_poseidon.h", "ministark_hip_hades_coin.h",
         "ministark_hip_blake3.h")
CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
RECORDS = {"ms_limb_spec": ("LimbSpecRecord", 32), "ms_range_set": ("RangeSetRecord", 16), "ms_limb_report": ("LimbReportRecord", 32)}


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
    assert sorted(_prototypes()) == NAMES                                       # exactly two prototypes
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.range_sigs) == NAMES
    others = (L.sigs, L.transcript_sigs, L.keccak_sigs, L.ext_sigs, L.logup_sigs, L.rpo_coin_sigs, L.lookup_sigs, L.sort_sigs, L.gap_sigs, L.join_sigs,
              L.poseidon_sigs, L.hades_coin_sigs, L.blake3_sigs)
    assert not any(set(NAMES) & set(o) for o in others)
    assert all(len(L.range_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    assert (len(L.range_sigs["ms_limb_decompose"][1]), len(L.range_sigs["ms_range_multiplicities"][1])) == (8, 11)
    assert all(getattr(L, n).argtypes == L.range_sigs[n][1] for n in NAMES)
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "ms_limb" not in text.lower() and "ms_range" not in text.lower(), older
    text = " ".join(_code().split())
    assert '#include "ministark_hip_ext.h"' in text and '#include "ministark_hip_lookup.h"' in text
    assert "MS_EXT_ALWAYS" not in text and "ms_lookup_report" not in text       # the mask kinds and the count's report are the other headers', not restated


def test_the_records_are_the_headers():
    from ministark_amd import _lib
    for name, (cls, size) in RECORDS.items():
        rec = getattr(_lib, cls)
        want = [(member, CTYPE[ctype]) for ctype, member in _members(name)]
        assert [(n, t) for n, t in rec._fields_] == want, name
        assert ctypes.sizeof(rec) == sum(ctypes.sizeof(t) for _, t in want) == size, name        # no padding the header does not spell out
    assert [m for _, m in _members("ms_limb_spec")] == ["src", "dst0", "nlimbs", "bits", "mask", "mask_col", "pad0", "pad1"]
    assert [m for _, m in _members("ms_range_set")] == ["col", "mask", "mask_col", "pad"]
    assert [m for _, m in _members("ms_limb_report")] == ["overflow", "first_overflow_row", "first_overflow_spec", "pad", "active"]
    host = open(os.path.join(ROOT, "ministark_amd", "csrc", "ms_range.cpp")).read()
    assert "sizeof(ms_limb_spec) == 32 && sizeof(ms_range_set) == 16 && sizeof(ms_limb_report) == 32" in host
    assert "sizeof(mslk::Report) == sizeof(ms_lookup_report)" in host


def test_the_python_constants_are_the_headers():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import extension
    assert dict(gen_rust_sys.header_enums(HEADER)) == {"MS_RANGE_MAX_SPECS": extension.RANGE_MAX_SPECS, "MS_RANGE_MAX_SETS": extension.RANGE_MAX_SETS,
                                                       "MS_RANGE_MAX_LIMBS": extension.RANGE_MAX_LIMBS, "MS_RANGE_MAX_LIMB_BITS": extension.RANGE_MAX_LIMB_BITS,
                                                       "MS_RANGE_MAX_TABLE_BITS": extension.RANGE_MAX_TABLE_BITS}
    assert (extension.RANGE_MAX_SPECS, extension.RANGE_MAX_SETS, extension.RANGE_MAX_LIMBS, extension.RANGE_MAX_LIMB_BITS, extension.RANGE_MAX_TABLE_BITS) == (64, 64, 256, 32, 24)


def test_the_kernels_take_their_atomics_and_their_finish_from_the_layers_below():
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    kernels = open(os.path.join(csrc, "range_kernels.h")).read()
    code = re.sub(r"//.*", "", kernels)
    assert '#include "direct_count.h"' in kernels and kernels.count("#include") == 1      # which brings lookup_kernels.h, which brings table_common.h
    shared = open(os.path.join(csrc, "direct_count.h")).read()
    shared_code = re.sub(r"//.*", "", shared)
    assert '#include "lookup_kernels.h"' in shared and shared.count("#include") == 1 and "atomic" not in shared_code and "extern __shared__" not in shared_code
    for fn in ("add", "amin"):
        assert "using mstab::%s;" % fn in kernels
    assert "atomic" not in code                                                 # every atomic goes through table_common.h, which the simulator makes exact
    assert "mslk::count_found<true>" in code and "mslk::from_count<F>" in code and "mstab::Canon<V>::words" in code
    assert "extern __shared__" not in code                                      # static shared memory only: the simulator has no dynamic kind
    assert "msdc::flush_bins<HB>" in code and "msdc::hist_add<HB>" in code and "msdc::hist_clear(" in code and "msdc::above<V>" in code and "msdc::limb_elem<F>" in code
    assert "mstab::block_totals(" in code and "mstab::FirstRow" in code and "mslk::write_report(" in code and "msdc::write_limb_report(" in code
    assert "static_assert(FLUSH_ROUNDS * LNT <= 65535" in code and "FLUSH_ROUNDS = msdc::FLUSH_ADDS;" in code
    assert "static_assert(FLUSH_ADDS * LNT <= 65535" in shared_code
    # each helper comes from exactly one layer below: defined once under csrc/, and not here
    texts = {f: re.sub(r"//.*", "", open(os.path.join(csrc, f)).read()) for f in os.listdir(csrc) if f.endswith((".h", ".cpp"))}
    for helper, home in (("flush_bins", "direct_count.h"), ("hist_add", "direct_count.h"), ("hist_clear", "direct_count.h"), ("above", "direct_count.h"),
                         ("limb_elem", "direct_count.h"), ("write_limb_report", "direct_count.h"), ("block_totals", "table_common.h"),
                         ("write_report", "lookup_kernels.h"), ("count_found", "lookup_kernels.h"), ("from_count", "lookup_kernels.h")):
        defined = [f for f, text in texts.items() if re.search(r"__forceinline__ [\w:<> ]+ %s\(" % helper, text)]
        assert defined == [home], (helper, defined)
    for record, home in (("FirstRow", "table_common.h"), ("LimbReport", "direct_count.h"), ("WriterParams", "direct_count.h")):
        assert [f for f, text in texts.items() if re.search(r"struct %s\b" % record, text)] == [home], record
    host = open(os.path.join(csrc, "ms_range.cpp")).read()
    assert "static_assert(msrg::MAXSPECS == (int)MS_RANGE_MAX_SPECS && msrg::MAXSETS == (int)MS_RANGE_MAX_SETS" in host
    assert '"MS_RANGE_FORM"' in host and "getenv(form_var)" in open(os.path.join(csrc, "count_args.h")).read()
    lookup = open(os.path.join(csrc, "lookup_kernels.h")).read()
    assert "msrg" not in lookup and "range" not in lookup.lower()               # the lookup layer does not know of this one
    for lower in ("direct_count.h", "lookup_kernels.h", "table_common.h"):      # nor does any layer below, outside the comments that say who uses it
        assert not re.search(r"msrg|msbw|range|bitwise", texts[lower].lower()), lower


def test_a_shared_helper_is_defined_once_and_no_kernel_is_renamed_by_the_preprocessor():
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".h", ".cpp"))}
    assert [f for f, text in texts.items() if re.search(r"\bvoid block_totals\(", text)] == ["table_common.h"]
    kernels = {m.group(1) for text in texts.values() for m in re.finditer(r"__global__\s+void\s+(?:__launch_bounds__\([^\n]*?\)\s+)?(\w+)\s*\(", text)}
    assert {"limb_finish", "limb_decompose", "range_count_lds", "bitwise_col_finish", "bitwise_count_lds", "join_finish", "lookup_finish"} <= kernels
    defined = {m.group(1) for text in texts.values() for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", text, flags=re.M)}
    assert not kernels & defined, sorted(kernels & defined)
    build = __import__("ministark_amd.build", fromlist=["SOURCES"])
    assert "ms_range.cpp" in build.SOURCES and HEADER in build._deps()


def test_sys_range_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.RANGE_OUT).read()
    assert text == gen_rust_sys.render_range(gen_rust_sys.range_prototypes())
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
    for const in ("MS_RANGE_MAX_SPECS: c_int = 64", "MS_RANGE_MAX_SETS: c_int = 64", "MS_RANGE_MAX_LIMBS: c_int = 256", "MS_RANGE_MAX_LIMB_BITS: c_int = 32",
                  "MS_RANGE_MAX_TABLE_BITS: c_int = 24"):
        assert "pub const " + const in text
    rust_type = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64"}
    for name in RECORDS:
        fields = ", ".join(f"pub {member}: {rust_type[ctype]}" for ctype, member in _members(name))
        assert f"pub struct {name} {{ {fields} }}" in text, name
    assert "pub mod sys_range;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.LOOKUP_OUT).read() == gen_rust_sys.render_lookup(gen_rust_sys.lookup_prototypes())
    assert open(gen_rust_sys.JOIN_OUT).read() == gen_rust_sys.render_join(gen_rust_sys.join_prototypes())
    assert open(gen_rust_sys.BLAKE3_OUT).read() == gen_rust_sys.render_blake3(gen_rust_sys.blake3_prototypes())
