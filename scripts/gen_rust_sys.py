#!/usr/bin/env python3
"""Generate rust/gpu/src/hip/sys.rs -- the raw `extern "C"` bindings of the reference-side shim -- from
include/ministark_hip.h, one Rust declaration per C prototype, sys_transcript.rs from include/ministark_hip_transcript.h, sys_keccak.rs from include/ministark_hip_keccak.h sys_ext.rs from include/ministark_hip_ext.h and sys_logup.rs from include/ministark_hip_logup.h, sys_rpo_coin.rs from include/ministark_hip_rpo_coin.h, sys_lookup.rs from include/ministark_hip_lookup.h, sys_sort.rs from include/ministark_hip_sort.h, sys_gaps.rs from include/ministark_hip_gaps.h, sys_join.rs from include/ministark_hip_join.h, sys_poseidon.rs from include/ministark_hip_poseidon.h, sys_hades_coin.rs from include/ministark_hip_hades_coin.h sys_blake3.rs from include/ministark_hip_blake3.h, sys_range.rs from include/ministark_hip_range.h and sys_bitwise.rs from include/ministark_hip_bitwise.h.  tests/test_rust_shim.py re-runs the parser and
checks the committed file against the header, which stands in for compiling it (no Rust toolchain in the image).

    python scripts/gen_rust_sys.py            # rewrite rust/gpu/src/hip/sys.rs
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ministark_hip.h")
OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys.rs")
TRANSCRIPT_HEADER = os.path.join(ROOT, "include", "ministark_hip_transcript.h")
TRANSCRIPT_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_transcript.rs")
KECCAK_HEADER = os.path.join(ROOT, "include", "ministark_hip_keccak.h")
KECCAK_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_keccak.rs")
EXT_HEADER = os.path.join(ROOT, "include", "ministark_hip_ext.h")
EXT_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_ext.rs")
LOGUP_HEADER = os.path.join(ROOT, "include", "ministark_hip_logup.h")
LOGUP_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_logup.rs")
RPO_COIN_HEADER = os.path.join(ROOT, "include", "ministark_hip_rpo_coin.h")
RPO_COIN_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_rpo_coin.rs")
LOOKUP_HEADER = os.path.join(ROOT, "include", "ministark_hip_lookup.h")
LOOKUP_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_lookup.rs")
SORT_HEADER = os.path.join(ROOT, "include", "ministark_hip_sort.h")
SORT_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_sort.rs")
GAPS_HEADER = os.path.join(ROOT, "include", "ministark_hip_gaps.h")
GAPS_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_gaps.rs")
JOIN_HEADER = os.path.join(ROOT, "include", "ministark_hip_join.h")
JOIN_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_join.rs")
POSEIDON_HEADER = os.path.join(ROOT, "include", "ministark_hip_poseidon.h")
POSEIDON_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_poseidon.rs")
HADES_COIN_HEADER = os.path.join(ROOT, "include", "ministark_hip_hades_coin.h")
HADES_COIN_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_hades_coin.rs")
BLAKE3_HEADER = os.path.join(ROOT, "include", "ministark_hip_blake3.h")
BLAKE3_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_blake3.rs")
RANGE_HEADER = os.path.join(ROOT, "include", "ministark_hip_range.h")
RANGE_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_range.rs")
BITWISE_HEADER = os.path.join(ROOT, "include", "ministark_hip_bitwise.h")
BITWISE_OUT = os.path.join(ROOT, "rust", "gpu", "src", "hip", "sys_bitwise.rs")

BASE = {"int": "c_int", "unsigned": "c_uint", "unsigned int": "c_uint", "long": "c_long", "size_t": "usize", "uint64_t": "u64",
        "uint32_t": "u32", "char": "c_char", "unsigned char": "u8", "void": "c_void", "ms_ctx": "ms_ctx", "ms_ntt_plan": "ms_ntt_plan", "ms_xchg_op": "ms_xchg_op", "ms_p2p_op": "ms_p2p_op", "ms_jit_stats": "ms_jit_stats"}
RUST_KEYWORDS = {"in", "type", "ref", "move", "fn", "use", "mod", "loop", "match", "next"}


def rust_type(ctype):
    """C declarator type (without the parameter name) -> Rust FFI type."""
    t = " ".join(ctype.replace("*", " * ").split())
    toks = t.split(" ")
    # peel pointers from the right: each '*' possibly followed by 'const'
    ptrs = []          # outermost last
    while toks and toks[-1] in ("*", "const"):
        if toks[-1] == "const":
            toks.pop()
            assert toks[-1] == "*", ctype
            toks.pop()
            ptrs.append("const_ptr_itself")      # `* const`: constness of the pointer variable, irrelevant for FFI
        else:
            toks.pop()
            ptrs.append("ptr")
    const_pointee = "const" in toks
    base = " ".join(x for x in toks if x != "const")
    r = BASE[base]
    # innermost pointer takes the pointee's constness; `T* const*` : outer pointer to const pointer -> *const *mut T
    levels = []
    seq = list(reversed(ptrs))                   # innermost first
    i = 0
    inner_const = const_pointee
    while i < len(seq):
        kind = seq[i]
        if kind == "ptr":
            levels.append(inner_const)
            inner_const = False
        else:                                    # this level is `* const`: the NEXT (outer) pointer points to a const pointer
            levels.append(inner_const)
            inner_const = True
        i += 1
    out = r
    for is_const in levels:
        out = ("*const " if is_const else "*mut ") + out
    return out


def prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = []
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        if "typedef" in ret:
            continue
        plist = []
        if params and params != "void":
            for p in params.split(","):
                p = p.strip()
                mm = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", p)
                ctype, pname = mm.group(1).strip(), mm.group(2)
                if ctype == "":                       # unnamed parameter
                    ctype, pname = p, f"arg{len(plist)}"
                plist.append((pname, rust_type(ctype)))
        protos.append((name, rust_type(ret) if ret != "void" else None, plist))
    return protos


def render(protos):
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip.h -- do not edit by hand.",
             "// Raw bindings of libministark_hip.so for the `hip` arm of crate ministark-gpu (INTEGRATION.md section 2).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_char, c_int, c_long, c_uint, c_void};",
             "",
             "#[repr(C)] pub struct ms_ctx { _private: [u8; 0] }",
             "#[repr(C)] pub struct ms_ntt_plan { _private: [u8; 0] }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_xchg_op { pub kind: u32, pub peer: u32, pub src_col: u32, pub dst_col: u32, pub src_offset: u64, pub bytes: u64 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug)] pub struct ms_p2p_op { pub kind: u32, pub peer: u32, pub d_ptr: *mut c_void, pub bytes: u64 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_jit_stats { pub kernels_compiled: u64, pub kernels_from_disk: u64, pub compile_failures: u64, pub damaged_entries: u64, pub compile_ms: f64, pub load_ms: f64 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_canon_report { pub count: u64, pub first_row: u64, pub first_col: u32, pub first_word: u32 }",
             "pub const MS_XCHG_SEND: u32 = 0;", "pub const MS_XCHG_RECV: u32 = 1;", "pub const MS_XCHG_COPY: u32 = 2;",
             "",
             "pub const MS_GOLDILOCKS_FP: c_int = 0;", "pub const MS_GOLDILOCKS_FQ3: c_int = 1;", "pub const MS_STARK252_FP: c_int = 2;",
             "pub const MS_OK: c_int = 0;", "pub const MS_ADD: c_int = 0;", "pub const MS_MUL: c_int = 1;",
             "pub const MS_NEG: c_int = 0;", "pub const MS_INV: c_int = 1;", "pub const MS_EXP: c_int = 2;",
             "pub const MS_EVAL_BIT_REVERSED: c_uint = 1;", "pub const MS_COMM_ID_BYTES: usize = 128;",
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", "",
              "/// The reference panics on every GPU-side failure (assert!/unwrap, gpu/src/plan.rs:248,255,360); keep that",
              "/// behaviour: never unwind across the FFI, panic on the Rust side with the library's message.",
              "pub fn check(rc: c_int) {",
              "    if rc != MS_OK {",
              "        let msg = unsafe { std::ffi::CStr::from_ptr(ms_last_error()) }.to_string_lossy().into_owned();",
              '        panic!("ministark_hip error {rc}: {msg}");',
              "    }",
              "}", ""]
    return "\n".join(lines)


def render_transcript(protos):
    """sys_transcript.rs: the entry points of include/ministark_hip_transcript.h (public coin, device-alpha fold), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_transcript.h -- do not edit by hand.",
             "// Raw bindings of the Fiat-Shamir layer of libministark_hip.so (INTEGRATION.md section 3c).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_coin_state { pub seed: [u8; 32], pub counter: u64, pub nbytes: u32, pub pad: u32, pub bytes: [u8; 32] }",
             "pub const MS_HASH_SHA256: c_int = 0;", "pub const MS_HASH_BLAKE2S: c_int = 1;",
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def transcript_prototypes():
    text = open(TRANSCRIPT_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_TRANSCRIPT_H"):])


def render_keccak(protos):
    """sys_keccak.rs: the entry points of include/ministark_hip_keccak.h (Keccak-256 / SHA3-256 commitments and proof-of-work), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_keccak.h -- do not edit by hand.",
             "// Raw bindings of the Keccak-256 / SHA3-256 layer of libministark_hip.so (INTEGRATION.md section 3d).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(KECCAK_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def header_enums(header):
    """the enumerators of a header's anonymous enums, in order: [(name, value)]"""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = []
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in body.split(","):
            name, value = (x.strip() for x in item.split("="))
            out.append((name, int(value, 0)))
    return out


def keccak_prototypes():
    text = open(KECCAK_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_KECCAK_H"):])


def render_ext(protos):
    """sys_ext.rs: the entry point of include/ministark_hip_ext.h (the extension columns between the two trace commitments), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_ext.h -- do not edit by hand.",
             "// Raw bindings of the extension-column layer of libministark_hip.so (INTEGRATION.md section 3e).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_ext_term { pub col: i32, pub off: i32, pub chal: i32, pub sign: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_ext_column { pub init: i32, pub init_chal: i32, pub mask: i32, pub mask_col: i32, pub inclusive: i32, pub na: u32, pub nb: u32, pub pad: u32 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(EXT_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def ext_prototypes():
    text = open(EXT_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_EXT_H"):])


def render_logup(protos):
    """sys_logup.rs: the entry point of include/ministark_hip_logup.h (LogUp lookup columns: running sums of fractions), on sys.rs's types;
    the terms, inits and masks are sys_ext.rs's"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_logup.h -- do not edit by hand.",
             "// Raw bindings of the LogUp-column layer of libministark_hip.so (INTEGRATION.md section 3e); ms_ext_term and the MS_EXT_* kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_logup_column { pub init: i32, pub init_chal: i32, pub mask: i32, pub mask_col: i32, pub inclusive: i32, pub nf: u32, pub pad0: u32, pub pad1: u32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_logup_fraction { pub nn: u32, pub nd: u32 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(LOGUP_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def logup_prototypes():
    text = open(LOGUP_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_LOGUP_H"):])


def render_rpo_coin(protos):
    """sys_rpo_coin.rs: the entry points of include/ministark_hip_rpo_coin.h (the RPO-256 public coin), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_rpo_coin.h -- do not edit by hand.",
             "// Raw bindings of the RPO-256 public coin of libministark_hip.so (INTEGRATION.md section 3f).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_rpo_coin_state { pub s: [u64; 12], pub pos: u32, pub pad: [u32; 7] }",
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def rpo_coin_prototypes():
    text = open(RPO_COIN_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_RPO_COIN_H"):])


def render_lookup(protos):
    """sys_lookup.rs: the entry point of include/ministark_hip_lookup.h (the multiplicity column of a LogUp lookup), on sys.rs's types; the
    mask kinds are sys_ext.rs's"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_lookup.h -- do not edit by hand.",
             "// Raw bindings of the lookup-multiplicity layer of libministark_hip.so (INTEGRATION.md section 3e); the MS_EXT_* mask kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_lookup_tuple { pub cols: [i32; 4], pub mask: i32, pub mask_col: i32, pub pad0: i32, pub pad1: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_lookup_report { pub missing: u64, pub first_missing_row: u64, pub first_missing_set: u32, pub pad: u32, pub duplicate_table_rows: u64 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(LOOKUP_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def lookup_prototypes():
    text = open(LOOKUP_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_LOOKUP_H"):])


def render_sort(protos):
    """sys_sort.rs: the entry points of include/ministark_hip_sort.h (the permutation that sorts trace rows, the gather by a device-resident
    index), on sys.rs's types; the mask kinds are sys_ext.rs's"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_sort.h -- do not edit by hand.",
             "// Raw bindings of the row-sort layer of libministark_hip.so (INTEGRATION.md section 3e); the MS_EXT_* mask kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_sort_key { pub cols: [i32; 4], pub mask: i32, pub mask_col: i32, pub pad0: i32, pub pad1: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_sort_report { pub active: u64, pub varying_bytes: u64 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(SORT_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def sort_prototypes():
    text = open(SORT_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_SORT_H"):])


def render_gaps(protos):
    """sys_gaps.rs: the entry points of include/ministark_hip_gaps.h (a padded table derived where the trace lies: select, fill clock gaps,
    pad), on sys.rs's types; the mask kinds are sys_ext.rs's"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_gaps.h -- do not edit by hand.",
             "// Raw bindings of the padded-table layer of libministark_hip.so (INTEGRATION.md section 3e); the MS_EXT_* mask kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_gap_spec { pub group: [i32; 3], pub ngroup: i32, pub counter: i32, pub mask: i32, pub mask_col: i32, pub pad0: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_gap_report { pub active: u64, pub rows_out: u64, pub gaps: u64, pub max_gap: u64, pub unordered: u64, pub first_unordered: u64, pub saturated: u64, pub pad0: u64 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_gap_column { pub kind: i32, pub src: i32 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(GAPS_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def gaps_prototypes():
    text = open(GAPS_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_GAPS_H"):])


def render_join(protos):
    """sys_join.rs: the entry point of include/ministark_hip_join.h (rows joined against a table: the matched row index), on sys.rs's types;
    the key record is sys_lookup.rs's ms_lookup_tuple and the mask kinds are sys_ext.rs's"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_join.h -- do not edit by hand.",
             "// Raw bindings of the row-join layer of libministark_hip.so (INTEGRATION.md section 3e); ms_lookup_tuple: sys_lookup.rs; the MS_EXT_* mask kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_join_report { pub matched: u64, pub missing: u64, pub first_missing_row: u64, pub first_missing_set: u32, pub pad: u32, pub duplicate_table_rows: u64, pub table_active: u64 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(JOIN_HEADER)] + [
             "pub const MS_JOIN_NONE: u32 = 0xFFFFFFFF;",
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def join_prototypes():
    text = open(JOIN_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_JOIN_H"):])


def render_poseidon(protos):
    """sys_poseidon.rs: the entry points of include/ministark_hip_poseidon.h (Starknet's Poseidon over the 252-bit field: the bulk
    permutation and the commitments), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_poseidon.h -- do not edit by hand.",
             "// Raw bindings of the Poseidon layer of libministark_hip.so (INTEGRATION.md section 3g).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def poseidon_prototypes():
    text = open(POSEIDON_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_POSEIDON_H"):])


def render_hades_coin(protos):
    """sys_hades_coin.rs: the entry points of include/ministark_hip_hades_coin.h (the Poseidon public coin of the 252-bit field), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_hades_coin.h -- do not edit by hand.",
             "// Raw bindings of the Poseidon public coin of the 252-bit field of libministark_hip.so (INTEGRATION.md section 3h).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_hades_coin_state { pub digest: [u64; 4], pub n_draws: u64, pub pad: [u32; 4] }",
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def hades_coin_prototypes():
    text = open(HADES_COIN_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_HADES_COIN_H"):])


def render_blake3(protos):
    """sys_blake3.rs: the entry points of include/ministark_hip_blake3.h (BLAKE3 commitments and proof-of-work), on sys.rs's types"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_blake3.h -- do not edit by hand.",
             "// Raw bindings of the BLAKE3 layer of libministark_hip.so (INTEGRATION.md section 3i).",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(BLAKE3_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def blake3_prototypes():
    text = open(BLAKE3_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_BLAKE3_H"):])


def render_range(protos):
    """sys_range.rs: the entry points of include/ministark_hip_range.h (range-check columns: limbs and direct-indexed multiplicities), on
    sys.rs's types; the count's report is sys_lookup.rs's ms_lookup_report and the mask kinds are sys_ext.rs's"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_range.h -- do not edit by hand.",
             "// Raw bindings of the range-check layer of libministark_hip.so (INTEGRATION.md section 3e); ms_lookup_report: sys_lookup.rs; the MS_EXT_* mask kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_limb_spec { pub src: i32, pub dst0: i32, pub nlimbs: i32, pub bits: i32, pub mask: i32, pub mask_col: i32, pub pad0: i32, pub pad1: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_range_set { pub col: i32, pub mask: i32, pub mask_col: i32, pub pad: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_limb_report { pub overflow: u64, pub first_overflow_row: u64, pub first_overflow_spec: u32, pub pad: u32, pub active: u64 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(RANGE_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def range_prototypes():
    text = open(RANGE_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_RANGE_H"):])


def render_bitwise(protos):
    """sys_bitwise.rs: the entry points of include/ministark_hip_bitwise.h (bitwise-operation columns, their table and its direct-indexed
    multiplicities), on sys.rs's types; the reports are sys_range.rs's ms_limb_report and sys_lookup.rs's ms_lookup_report"""
    lines = ["// GENERATED by scripts/gen_rust_sys.py from include/ministark_hip_bitwise.h -- do not edit by hand.",
             "// Raw bindings of the bitwise-operation layer of libministark_hip.so (INTEGRATION.md section 3e); ms_limb_report: sys_range.rs; ms_lookup_report: sys_lookup.rs; the MS_EXT_* mask kinds: sys_ext.rs.",
             "#![allow(non_camel_case_types)]",
             "use core::ffi::{c_int, c_uint, c_void};",
             "use super::sys::ms_ctx;",
             "",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_bitwise_spec { pub op: i32, pub a: i32, pub b: i32, pub dst: i32, pub width: i32, pub mask: i32, pub mask_col: i32, pub pad: i32 }",
             "#[repr(C)] #[derive(Clone, Copy, Debug, Default)] pub struct ms_bitwise_set { pub op: i32, pub a: i32, pub b: i32, pub c: i32, pub nlimbs: i32, pub mask: i32, pub mask_col: i32, pub pad: i32 }",
             ] + [f"pub const {name}: c_int = {value};" for name, value in header_enums(BITWISE_HEADER)] + [
             "",
             '#[link(name = "ministark_hip")]', 'extern "C" {']
    for name, ret, plist in protos:
        args = ", ".join(f"{(p + '_') if p in RUST_KEYWORDS else p}: {t}" for p, t in plist)
        lines.append(f"    pub fn {name}({args})" + (f" -> {ret};" if ret else ";"))
    lines += ["}", ""]
    return "\n".join(lines)


def bitwise_prototypes():
    text = open(BITWISE_HEADER).read()
    return prototypes(text[text.index("#define MINISTARK_HIP_BITWISE_H"):])


def main():
    protos = prototypes(open(HEADER).read())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(render(protos))
    print(f"{len(protos)} prototypes -> {OUT}")
    protos = transcript_prototypes()
    with open(TRANSCRIPT_OUT, "w") as f:
        f.write(render_transcript(protos))
    print(f"{len(protos)} prototypes -> {TRANSCRIPT_OUT}")
    protos = keccak_prototypes()
    with open(KECCAK_OUT, "w") as f:
        f.write(render_keccak(protos))
    print(f"{len(protos)} prototypes -> {KECCAK_OUT}")
    protos = ext_prototypes()
    with open(EXT_OUT, "w") as f:
        f.write(render_ext(protos))
    print(f"{len(protos)} prototypes -> {EXT_OUT}")
    protos = logup_prototypes()
    with open(LOGUP_OUT, "w") as f:
        f.write(render_logup(protos))
    print(f"{len(protos)} prototypes -> {LOGUP_OUT}")
    protos = rpo_coin_prototypes()
    with open(RPO_COIN_OUT, "w") as f:
        f.write(render_rpo_coin(protos))
    print(f"{len(protos)} prototypes -> {RPO_COIN_OUT}")
    protos = lookup_prototypes()
    with open(LOOKUP_OUT, "w") as f:
        f.write(render_lookup(protos))
    print(f"{len(protos)} prototypes -> {LOOKUP_OUT}")
    protos = sort_prototypes()
    with open(SORT_OUT, "w") as f:
        f.write(render_sort(protos))
    print(f"{len(protos)} prototypes -> {SORT_OUT}")
    protos = gaps_prototypes()
    with open(GAPS_OUT, "w") as f:
        f.write(render_gaps(protos))
    print(f"{len(protos)} prototypes -> {GAPS_OUT}")
    protos = join_prototypes()
    with open(JOIN_OUT, "w") as f:
        f.write(render_join(protos))
    print(f"{len(protos)} prototypes -> {JOIN_OUT}")
    protos = poseidon_prototypes()
    with open(POSEIDON_OUT, "w") as f:
        f.write(render_poseidon(protos))
    print(f"{len(protos)} prototypes -> {POSEIDON_OUT}")
    protos = hades_coin_prototypes()
    with open(HADES_COIN_OUT, "w") as f:
        f.write(render_hades_coin(protos))
    print(f"{len(protos)} prototypes -> {HADES_COIN_OUT}")
    protos = blake3_prototypes()
    with open(BLAKE3_OUT, "w") as f:
        f.write(render_blake3(protos))
    print(f"{len(protos)} prototypes -> {BLAKE3_OUT}")
    protos = range_prototypes()
    with open(RANGE_OUT, "w") as f:
        f.write(render_range(protos))
    print(f"{len(protos)} prototypes -> {RANGE_OUT}")
    protos = bitwise_prototypes()
    with open(BITWISE_OUT, "w") as f:
        f.write(render_bitwise(protos))
    print(f"{len(protos)} prototypes -> {BITWISE_OUT}")


if __name__ == "__main__":
    main()
