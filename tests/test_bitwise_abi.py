"""include/ministark_hip_bitwise.h -- bitwise-operation columns -- against what binds it: the library exports the symbols it declares,
`_lib.Lib.bitwise_sigs` declares the same, rust/gpu/src/hip/sys_bitwise.rs is what the generator writes and agrees with the header through
test_rust_shim's independent C -> Rust type table, the record layouts and enum values are the ones the Python mirror packs and the kernels
assume, and the older headers name none of it."""
import ctypes
import os
import re
import subprocess
import sys

from tests.test_rust_shim import _expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip_bitwise.h")
NAMES = ["ms_bitwise_columns", "ms_bitwise_multiplicities", "ms_bitwise_table"]
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h", "ministark_hip_logup.h", "ministark_hip_rpo_coin.h",
         "ministark_hip_lookup.h", "ministark_hip_sort.h", "ministark_hip_gaps.h", "ministark_hip_join.h", "ministark_hip_poseidon.h", "ministark_hip_hades_coin.h",
         "ministark_hip_blake3.h", "ministark_hip_range.h")
CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
RECORDS = {"ms_bitwise_spec": ("BitwiseSpecRecord", 32), "ms_bitwise_set": ("BitwiseSetRecord", 32)}
ENUMS = {"MS_BIT_AND": 0, "MS_BIT_OR": 1, "MS_BIT_XOR": 2, "MS_BITWISE_MAX_SPECS": 64, "MS_BITWISE_MAX_SETS": 64, "MS_BITWISE_MAX_LIMBS": 256, "MS_BITWISE_MAX_BITS": 12,
         "MS_BITWISE_MAX_OPS": 3, "MS_BITWISE_MAX_TABLE_LOG": 24}


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
    assert sorted(_prototypes()) == NAMES                                       # exactly three prototypes
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.bitwise_sigs) == NAMES
    others = (L.sigs, L.transcript_sigs, L.keccak_sigs, L.ext_sigs, L.logup_sigs, L.rpo_coin_sigs, L.lookup_sigs, L.sort_sigs, L.gap_sigs, L.join_sigs,
              L.poseidon_sigs, L.hades_coin_sigs, L.blake3_sigs, L.range_sigs)
    assert not any(set(NAMES) & set(o) for o in others)
    assert all(len(L.bitwise_sigs[n][1]) == len(params) for n, params in _prototypes().items())
    assert [len(L.bitwise_sigs[n][1]) for n in NAMES] == [8, 13, 10]
    assert all(getattr(L, n).argtypes == L.bitwise_sigs[n][1] for n in NAMES)
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "ms_bitwise" not in text.lower() and "ms_bit_and" not in text.lower(), older
    text = " ".join(_code().split())
    assert '#include "ministark_hip_range.h"' in text
    assert "MS_EXT_ALWAYS" not in text and "ms_lookup_report" not in text and "ms_limb_report" not in text      # the masks and both reports are the other headers', not restated


def test_the_records_are_the_headers():
    from ministark_amd import _lib
    for name, (cls, size) in RECORDS.items():
        rec = getattr(_lib, cls)
        want = [(member, CTYPE[ctype]) for ctype, member in _members(name)]
        assert [(n, t) for n, t in rec._fields_] == want, name
        assert ctypes.sizeof(rec) == sum(ctypes.sizeof(t) for _, t in want) == size, name        # no padding the header does not spell out
    assert [m for _, m in _members("ms_bitwise_spec")] == ["op", "a", "b", "dst", "width", "mask", "mask_col", "pad"]
    assert [m for _, m in _members("ms_bitwise_set")] == ["op", "a", "b", "c", "nlimbs", "mask", "mask_col", "pad"]
    host = open(os.path.join(ROOT, "ministark_amd", "csrc", "ms_bitwise.cpp")).read()
    assert "sizeof(ms_bitwise_spec) == 32 && sizeof(ms_bitwise_set) == 32" in host and "sizeof(msdc::LimbReport) == sizeof(ms_limb_report)" in host


def test_the_python_constants_are_the_headers():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    from ministark_amd import GOLDILOCKS_FP, STARK252_FP, extension
    assert dict(gen_rust_sys.header_enums(HEADER)) == ENUMS
    assert extension.BITWISE_OPS == {"and": ENUMS["MS_BIT_AND"], "or": ENUMS["MS_BIT_OR"], "xor": ENUMS["MS_BIT_XOR"]}
    assert (extension.BITWISE_MAX_SPECS, extension.BITWISE_MAX_SETS, extension.BITWISE_MAX_LIMBS, extension.BITWISE_MAX_BITS, extension.BITWISE_MAX_OPS,
            extension.BITWISE_MAX_TABLE_LOG) == tuple(ENUMS[k] for k in ("MS_BITWISE_MAX_SPECS", "MS_BITWISE_MAX_SETS", "MS_BITWISE_MAX_LIMBS", "MS_BITWISE_MAX_BITS",
                                                                         "MS_BITWISE_MAX_OPS", "MS_BITWISE_MAX_TABLE_LOG"))
    # 2^WMAX is the widest power of two below the modulus
    from tests.ext_ref import PAIRS
    assert all(1 << extension.BITWISE_WMAX[f] < PAIRS[k].bf.p < 2 << extension.BITWISE_WMAX[f] for f, k in ((GOLDILOCKS_FP, "fp_fp"), (STARK252_FP, "fp252_fp252")))


def test_the_kernels_take_their_atomics_and_their_helpers_from_the_layers_below():
    csrc = os.path.join(ROOT, "ministark_amd", "csrc")
    kernels = open(os.path.join(csrc, "bitwise_kernels.h")).read()
    code = re.sub(r"//.*", "", kernels)
    assert '#include "direct_count.h"' in kernels and kernels.count("#include") == 1      # which brings lookup_kernels.h, which brings table_common.h
    assert '"range_kernels.h"' not in code and "msrg" not in code and "#define" not in code      # the sibling unit's header is not this one's layer below
    for fn in ("add", "amin"):
        assert "using mstab::%s;" % fn in kernels
    assert "atomic" not in code                                                 # every atomic goes through table_common.h, which the simulator makes exact
    assert "mslk::count_found<true>" in code and "mslk::from_count<F>" in code and "mstab::Canon<V>::words" in code
    assert "msdc::flush_bins<HB>" in code and "msdc::hist_add<HB>" in code and "msdc::hist_clear(" in code and "msdc::above<V>" in code and "msdc::limb_elem<F>" in code
    assert "mstab::block_totals(" in code and "mstab::FirstRow" in code and "mslk::write_report(" in code and "msdc::write_limb_report(" in code
    for helper in ("flush_bins", "hist_add", "hist_clear", "above", "limb_elem", "block_totals", "write_report", "write_limb_report", "count_found", "from_count"):
        assert not re.search(r"__forceinline__ [\w:<> ]+ %s\(" % helper, code), helper      # taken from below (tests/test_range_abi.py: defined once), not restated
    assert "extern __shared__" not in code                                      # static shared memory only: the simulator has no dynamic kind
    assert "static_assert(FLUSH_INCS * LNT <= 65535" in code and "static_assert(PACKED_MAX_LIMBS <= FLUSH_INCS" in code and "FLUSH_INCS = msdc::FLUSH_ADDS;" in code
    host = open(os.path.join(csrc, "ms_bitwise.cpp")).read()
    assert "static_assert(msbw::MAXSPECS == (int)MS_BITWISE_MAX_SPECS && msbw::MAXSETS == (int)MS_BITWISE_MAX_SETS" in host
    assert '"MS_BITWISE_FORM"' in host and "getenv(form_var)" in open(os.path.join(csrc, "count_args.h")).read()
    text = open(os.path.join(csrc, "lookup_kernels.h")).read()
    assert "msbw" not in text and "bitwise" not in text.lower()                 # the layers below do not know of this one
    for lower in ("direct_count.h", "lookup_kernels.h", "table_common.h"):      # outside the comments that say who uses them
        assert not re.search(r"msrg|msbw|range|bitwise", re.sub(r"//.*", "", open(os.path.join(csrc, lower)).read()).lower()), lower
    sibling = open(os.path.join(csrc, "range_kernels.h")).read()
    assert "msbw" not in sibling and "bitwise" not in sibling.lower()           # nor does the sibling unit
    build = __import__("ministark_amd.build", fromlist=["SOURCES"])
    assert "ms_bitwise.cpp" in build.SOURCES and HEADER in build._deps()


def test_sys_bitwise_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.BITWISE_OUT).read()
    assert text == gen_rust_sys.render_bitwise(gen_rust_sys.bitwise_prototypes())
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
    for const, value in ENUMS.items():
        assert f"pub const {const}: c_int = {value};" in text
    rust_type = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64"}
    for name in RECORDS:
        fields = ", ".join(f"pub {member}: {rust_type[ctype]}" for ctype, member in _members(name))
        assert f"pub struct {name} {{ {fields} }}" in text, name
    assert "pub mod sys_bitwise;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.RANGE_OUT).read() == gen_rust_sys.render_range(gen_rust_sys.range_prototypes())
    assert open(gen_rust_sys.LOOKUP_OUT).read() == gen_rust_sys.render_lookup(gen_rust_sys.lookup_prototypes())


def test_every_barrier_of_the_lds_count_waits_for_the_lds_adds_before_it(tmp_path):
    """The gfx950 assembly of bitwise_count_lds: before every s_barrier, with nothing but arithmetic in between, stands a wait for the
    wave's outstanding LDS operations.  A first build, whose flush check stood in front of a row's adds, came out of the compiler without that wait before the
    flush's first barrier, and on the device an add that landed between a lane's read of a histogram word and its clearing of it was lost:
    a few counts in 10^8, on a hot bin, not on every run -- nothing a test of 2500 rows sees."""
    from ministark_amd import build
    out = str(tmp_path / "ms_bitwise.s")
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "ms_bitwise.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    kernels = re.findall(r"^(_ZN4msbw17bitwise_count_lds\w+):[^\n]*\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert len(kernels) == 6                                                    # V = 1, 4 by HB = 12, 14, 16
    for name, body in kernels:
        ins = [line.split(";")[0].strip() for line in body.split("\n")]
        ins = [i for i in ins if i and not (i.startswith(".") and not i.endswith(":"))]
        barriers = [k for k, i in enumerate(ins) if i.startswith("s_barrier")]
        assert len(barriers) >= 3, name                                         # after the clearing, and the two of a flush
        for k in barriers:
            j = k - 1                                                           # back over arithmetic alone: no LDS operation, branch or label in between
            while j >= 0 and not ins[j].startswith(("s_waitcnt", "ds_", "s_cbranch", "s_branch")) and not ins[j].endswith(":"):
                j -= 1
            assert j >= 0 and ins[j].startswith("s_waitcnt") and "lgkmcnt(0)" in ins[j], (name, ins[max(0, j - 2):k + 1])
