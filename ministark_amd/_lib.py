"""ctypes loader for libministark_hip.so -- the ONLY native library the package loads.

There is no CPU fallback: if the hipcc-built library is missing, or no AMD GPU is
visible when a context is created, this raises.  (tests/emu builds a g++ simulator
of the same sources for kernel-logic tests; that library is loaded by the tests
through `Lib(path)` explicitly and is never looked for here.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SO = os.path.join(_HERE, "libministark_hip.so")

c_void_pp = ctypes.POINTER(ctypes.c_void_p)


class MsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ministark_hip error {code}: {msg}")
        self.code = code


class JitStats(ctypes.Structure):
    """`ms_jit_stats` of include/ministark_hip.h."""
    _fields_ = [("kernels_compiled", ctypes.c_uint64), ("kernels_from_disk", ctypes.c_uint64), ("compile_failures", ctypes.c_uint64),
                ("damaged_entries", ctypes.c_uint64), ("compile_ms", ctypes.c_double), ("load_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CanonReport(ctypes.Structure):
    """`ms_canon_report` of include/ministark_hip.h: what ms_check_canonical found."""
    _fields_ = [("count", ctypes.c_uint64), ("first_row", ctypes.c_uint64), ("first_col", ctypes.c_uint32), ("first_word", ctypes.c_uint32)]

    def __bool__(self):
        return self.count == 0                   # true when every element is canonical

    def __repr__(self):
        if not self.count:
            return "CanonReport(count=0)"
        return f"CanonReport(count={self.count}, first_col={self.first_col}, first_row={self.first_row}, first_word={self.first_word})"


class CoinState(ctypes.Structure):
    """`ms_coin_state` of include/ministark_hip_transcript.h: the public coin's seed, counter and unread bytes."""
    _fields_ = [("seed", ctypes.c_uint8 * 32), ("counter", ctypes.c_uint64), ("nbytes", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("bytes", ctypes.c_uint8 * 32)]


class HadesCoinState(ctypes.Structure):
    """`ms_hades_coin_state` of include/ministark_hip_hades_coin.h: the Poseidon coin's digest (Montgomery words) and its draw counter."""
    _fields_ = [("digest", ctypes.c_uint64 * 4), ("n_draws", ctypes.c_uint64), ("pad", ctypes.c_uint32 * 4)]


class RpoCoinState(ctypes.Structure):
    """`ms_rpo_coin_state` of include/ministark_hip_rpo_coin.h: the RPO-256 coin's sponge (Montgomery words) and its read position."""
    _fields_ = [("s", ctypes.c_uint64 * 12), ("pos", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 7)]


class LookupReportRecord(ctypes.Structure):
    """`ms_lookup_report` of include/ministark_hip_lookup.h: what ms_lookup_multiplicities found."""
    _fields_ = [("missing", ctypes.c_uint64), ("first_missing_row", ctypes.c_uint64), ("first_missing_set", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("duplicate_table_rows", ctypes.c_uint64)]


class LookupTupleRecord(ctypes.Structure):
    """`ms_lookup_tuple` of include/ministark_hip_lookup.h."""
    _fields_ = [("cols", ctypes.c_int32 * 4), ("mask", ctypes.c_int32), ("mask_col", ctypes.c_int32), ("pad0", ctypes.c_int32), ("pad1", ctypes.c_int32)]


class JoinReportRecord(ctypes.Structure):
    """`ms_join_report` of include/ministark_hip_join.h: what ms_join_rows found."""
    _fields_ = [("matched", ctypes.c_uint64), ("missing", ctypes.c_uint64), ("first_missing_row", ctypes.c_uint64), ("first_missing_set", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("duplicate_table_rows", ctypes.c_uint64), ("table_active", ctypes.c_uint64)]


class LimbSpecRecord(ctypes.Structure):
    """`ms_limb_spec` of include/ministark_hip_range.h."""
    _fields_ = [("src", ctypes.c_int32), ("dst0", ctypes.c_int32), ("nlimbs", ctypes.c_int32), ("bits", ctypes.c_int32), ("mask", ctypes.c_int32), ("mask_col", ctypes.c_int32),
                ("pad0", ctypes.c_int32), ("pad1", ctypes.c_int32)]


class RangeSetRecord(ctypes.Structure):
    """`ms_range_set` of include/ministark_hip_range.h."""
    _fields_ = [("col", ctypes.c_int32), ("mask", ctypes.c_int32), ("mask_col", ctypes.c_int32), ("pad", ctypes.c_int32)]


class LimbReportRecord(ctypes.Structure):
    """`ms_limb_report` of include/ministark_hip_range.h: what ms_limb_decompose found."""
    _fields_ = [("overflow", ctypes.c_uint64), ("first_overflow_row", ctypes.c_uint64), ("first_overflow_spec", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("active", ctypes.c_uint64)]


class BitwiseSpecRecord(ctypes.Structure):
    """`ms_bitwise_spec` of include/ministark_hip_bitwise.h."""
    _fields_ = [("op", ctypes.c_int32), ("a", ctypes.c_int32), ("b", ctypes.c_int32), ("dst", ctypes.c_int32), ("width", ctypes.c_int32), ("mask", ctypes.c_int32),
                ("mask_col", ctypes.c_int32), ("pad", ctypes.c_int32)]


class BitwiseSetRecord(ctypes.Structure):
    """`ms_bitwise_set` of include/ministark_hip_bitwise.h."""
    _fields_ = [("op", ctypes.c_int32), ("a", ctypes.c_int32), ("b", ctypes.c_int32), ("c", ctypes.c_int32), ("nlimbs", ctypes.c_int32), ("mask", ctypes.c_int32),
                ("mask_col", ctypes.c_int32), ("pad", ctypes.c_int32)]


class SortKeyRecord(ctypes.Structure):
    """`ms_sort_key` of include/ministark_hip_sort.h."""
    _fields_ = [("cols", ctypes.c_int32 * 4), ("mask", ctypes.c_int32), ("mask_col", ctypes.c_int32), ("pad0", ctypes.c_int32), ("pad1", ctypes.c_int32)]


class SortReportRecord(ctypes.Structure):
    """`ms_sort_report` of include/ministark_hip_sort.h: what ms_sort_rows found."""
    _fields_ = [("active", ctypes.c_uint64), ("varying_bytes", ctypes.c_uint64)]


class GapSpecRecord(ctypes.Structure):
    """`ms_gap_spec` of include/ministark_hip_gaps.h."""
    _fields_ = [("group", ctypes.c_int32 * 3), ("ngroup", ctypes.c_int32), ("counter", ctypes.c_int32), ("mask", ctypes.c_int32), ("mask_col", ctypes.c_int32), ("pad0", ctypes.c_int32)]


class GapReportRecord(ctypes.Structure):
    """`ms_gap_report` of include/ministark_hip_gaps.h: what ms_gap_plan found."""
    _fields_ = [("active", ctypes.c_uint64), ("rows_out", ctypes.c_uint64), ("gaps", ctypes.c_uint64), ("max_gap", ctypes.c_uint64), ("unordered", ctypes.c_uint64),
                ("first_unordered", ctypes.c_uint64), ("saturated", ctypes.c_uint64), ("pad0", ctypes.c_uint64)]


class GapColumnRecord(ctypes.Structure):
    """`ms_gap_column` of include/ministark_hip_gaps.h."""
    _fields_ = [("kind", ctypes.c_int32), ("src", ctypes.c_int32)]


class Lib:
    """Typed view of the C ABI in include/ministark_hip.h."""

    def __init__(self, path=None):
        path = path or DEFAULT_SO
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: build it with `python -m ministark_amd.build` (hipcc, gfx950). "
                "There is no CPU fallback.")
        self.path = path
        L = ctypes.CDLL(path)
        self.L = L
        vp, u, i, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t
        sigs = {
            "ms_ctx_create": (i, [i, c_void_pp]),
            "ms_ctx_destroy": (i, [vp]),
            "ms_sync": (i, [vp]),
            "ms_ctx_stream": (vp, [vp]),
            "ms_last_error": (ctypes.c_char_p, []),
            "ms_field_bytes": (sz, [i]),
            "ms_profile_enable": (i, [vp, i]),
            "ms_profile_read": (i, [vp, ctypes.c_char_p, sz]),
            "ms_check_canonical": (i, [vp, i, sz, c_void_pp, u, vp]),
            "ms_check_canonical_host": (i, [i, vp, sz, ctypes.POINTER(sz)]),
            "ms_ctx_set_checked": (i, [vp, i]),
            "ms_ctx_get_checked": (i, [vp, ctypes.POINTER(i)]),
            "ms_alloc": (i, [vp, sz, c_void_pp]),
            "ms_free": (i, [vp, vp]),
            "ms_copy": (i, [vp, vp, vp, sz]),
            "ms_upload": (i, [vp, vp, vp, sz]),
            "ms_download": (i, [vp, vp, vp, sz]),
            "ms_ntt_plan_create": (i, [vp, i, u, i, vp, vp, c_void_pp]),
            "ms_ntt_plan_destroy": (i, [vp]),
            "ms_ntt_encode": (i, [vp, vp]),
            "ms_ntt_execute": (i, [vp]),
            "ms_ntt_enqueue": (i, [vp, c_void_pp, u]),
            "ms_ntt_enqueue_to": (i, [vp, c_void_pp, c_void_pp, u]),
            "ms_bit_reverse": (i, [vp, i, u, c_void_pp, u]),
            "ms_lde": (i, [vp, i, u, u, vp, c_void_pp, c_void_pp, u, i]),
            "ms_evaluate": (i, [vp, i, u, u, vp, c_void_pp, c_void_pp, u, i]),
            "ms_deinterleave": (i, [vp, i, sz, u, vp, c_void_pp]),
            "ms_binary": (i, [vp, i, i, i, sz, vp, vp, vp, ctypes.c_long]),
            "ms_binary_const": (i, [vp, i, i, i, sz, vp, vp, vp]),
            "ms_mul_pow": (i, [vp, i, i, sz, vp, vp, vp, u, ctypes.c_long]),
            "ms_unary": (i, [vp, i, i, sz, vp, vp, u]),
            "ms_convert": (i, [vp, i, i, sz, vp, vp]),
            "ms_fill": (i, [vp, i, sz, vp, vp]),
            "ms_sum_columns": (i, [vp, i, sz, c_void_pp, u, vp]),
            "ms_eval_program": (i, [vp, vp, u, vp, u, u, u, vp, vp, c_void_pp, u, c_void_pp, u, c_void_pp, vp, u, i, vp]),
            "ms_eval_program_ex": (i, [vp, vp, u, vp, u, u, u, vp, vp, c_void_pp, u, c_void_pp, u, c_void_pp, vp, u, i, vp, u]),
            "ms_validate_constraints": (i, [vp, i, vp, u, vp, u, u, c_void_pp, u, c_void_pp, u, c_void_pp, vp, u, u, vp, vp]),
            "ms_eval_jit_check": (i, [vp, u, i, vp]),
            "ms_eval_jit_stats": (i, [vp, ctypes.POINTER(JitStats)]),
            "ms_scan_affine": (i, [vp, i, sz, vp, vp, vp, i, vp]),
            "ms_gather_rows": (i, [vp, i, sz, c_void_pp, u, vp, sz, vp]),
            "ms_gather_digests": (i, [vp, sz, vp, vp, sz, vp]),
            "ms_gather_digests_multi": (i, [vp, u, c_void_pp, ctypes.POINTER(sz), vp, ctypes.POINTER(sz), c_void_pp]),
            "ms_merkle_view_ids": (i, [sz, vp, sz, vp, vp, vp, vp, vp]),
            "ms_fri_fold": (i, [vp, i, u, u, vp, vp, vp, vp]),
            "ms_fri_fold_rows": (i, [vp, i, u, u, vp, vp, sz, sz, vp, vp]),
            "ms_sha256_rows": (i, [vp, i, sz, c_void_pp, u, vp]),
            "ms_sha256_merkle": (i, [vp, sz, vp, vp]),
            "ms_horner_eval": (i, [vp, i, i, sz, c_void_pp, u, vp, vp, u, vp]),
            "ms_deep_compose": (i, [vp, i, u, vp, c_void_pp, u, c_void_pp, u, vp, u, vp, vp, vp, vp, u, vp, vp, vp]),
            "ms_deep_rows": (i, [vp, i, u, vp, sz, sz, c_void_pp, u, c_void_pp, u, vp, u, vp, vp, vp, vp, u, vp, vp, vp]),
            "ms_sha256_pow_grind": (i, [vp, vp, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
            "ms_rpo256_rows": (i, [vp, sz, c_void_pp, u, vp]),
            "ms_rpo256_rows_row_major": (i, [vp, sz, u, vp, vp]),
            "ms_rpo256_merkle": (i, [vp, sz, vp, vp]),
            "ms_rpo256_rows_field": (i, [vp, i, sz, c_void_pp, u, vp]),
            "ms_blake2s_rows": (i, [vp, i, sz, c_void_pp, u, vp]),
            "ms_blake2s_rows_row_major": (i, [vp, i, sz, u, vp, vp]),
            "ms_blake2s_merkle": (i, [vp, sz, vp, vp]),
            "ms_blake2s_pow_grind": (i, [vp, vp, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
            "ms_comm_unique_id": (i, [vp]),
            "ms_comm_init": (i, [vp, i, i, vp]),
            "ms_comm_destroy": (i, [vp]),
            "ms_comm_rank": (i, [vp, ctypes.POINTER(i), ctypes.POINTER(i)]),
            "ms_cols_to_rows_alltoall": (i, [vp, i, sz, c_void_pp, u, u, c_void_pp]),
            "ms_allgather_digests": (i, [vp, vp, vp]),
            "ms_cols_to_rows_schedule": (i, [u, u, u, u, sz, vp, sz, ctypes.POINTER(sz)]),
            "ms_p2p_batch": (i, [vp, vp, sz]),
            "ms_sha256_rows_row_major": (i, [vp, i, sz, u, vp, vp]),
        }
        # include/ministark_hip_transcript.h: the device-resident public coin and the fold that reads its challenge on the device
        transcript_sigs = {
            "ms_fri_fold_dev": (i, [vp, i, u, u, vp, vp, vp, vp]),
            "ms_coin_create": (i, [vp, i, vp, c_void_pp]),
            "ms_coin_destroy": (i, [vp, vp]),
            "ms_coin_read": (i, [vp, vp, vp]),
            "ms_coin_write": (i, [vp, vp, vp]),
            "ms_coin_reseed_digest": (i, [vp, vp, vp]),
            "ms_coin_reseed_int": (i, [vp, vp, ctypes.c_uint64]),
            "ms_coin_reseed_elements": (i, [vp, vp, i, vp, sz]),
            "ms_coin_reseed_elements_host": (i, [vp, vp, i, vp, sz]),
            "ms_coin_draw": (i, [vp, vp, i, sz, vp]),
            "ms_coin_draw_queries": (i, [vp, vp, sz, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(sz)]),
            "ms_coin_pow_grind": (i, [vp, vp, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        }
        # include/ministark_hip_keccak.h: Keccak-256 / SHA3-256 commitments and proof-of-work (`variant` after the context)
        keccak_sigs = {
            "ms_keccak_rows": (i, [vp, i, i, sz, c_void_pp, u, vp]),
            "ms_keccak_rows_row_major": (i, [vp, i, i, sz, u, vp, vp]),
            "ms_keccak_merkle": (i, [vp, i, sz, vp, vp]),
            "ms_keccak_pow_grind": (i, [vp, i, vp, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        }
        # include/ministark_hip_blake3.h: BLAKE3 commitments and proof-of-work, each the twin of its ms_blake2s_* namesake
        blake3_sigs = {
            "ms_blake3_rows": (i, [vp, i, sz, c_void_pp, u, vp]),
            "ms_blake3_rows_row_major": (i, [vp, i, sz, u, vp, vp]),
            "ms_blake3_merkle": (i, [vp, sz, vp, vp]),
            "ms_blake3_pow_grind": (i, [vp, vp, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        }
        # include/ministark_hip_ext.h: the extension columns between the two trace commitments
        ext_sigs = {
            "ms_build_extension_columns": (i, [vp, i, i, sz, c_void_pp, u, vp, u, vp, vp, u, c_void_pp]),
        }
        # include/ministark_hip_logup.h: the LogUp lookup columns (running sums of fractions)
        logup_sigs = {
            "ms_build_logup_columns": (i, [vp, i, i, sz, c_void_pp, u, vp, u, vp, vp, vp, u, c_void_pp]),
        }
        # include/ministark_hip_rpo_coin.h and include/ministark_hip_hades_coin.h: the two algebraic public coins, each entry point the twin of its
        # ms_coin_* namesake, minus `hash`
        def algebraic_coin_sigs(prefix):
            return {prefix + name: sig for name, sig in {
                "create": (i, [vp, vp, c_void_pp]),
                "destroy": (i, [vp, vp]),
                "read": (i, [vp, vp, vp]),
                "write": (i, [vp, vp, vp]),
                "reseed_digest": (i, [vp, vp, vp]),
                "reseed_int": (i, [vp, vp, ctypes.c_uint64]),
                "reseed_elements": (i, [vp, vp, i, vp, sz]),
                "reseed_elements_host": (i, [vp, vp, i, vp, sz]),
                "draw": (i, [vp, vp, i, sz, vp]),
                "draw_queries": (i, [vp, vp, sz, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(sz)]),
                "pow_grind": (i, [vp, vp, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
            }.items()}
        rpo_coin_sigs = algebraic_coin_sigs("ms_rpo_coin_")
        hades_coin_sigs = algebraic_coin_sigs("ms_hades_coin_")
        # include/ministark_hip_lookup.h: the multiplicity column of a LogUp lookup, counted on the device
        lookup_sigs = {
            "ms_lookup_multiplicities": (i, [vp, i, sz, c_void_pp, u, u, vp, vp, u, vp, vp]),
        }
        # include/ministark_hip_sort.h: the permutation that sorts trace rows, and a gather by a device-resident index
        sort_sigs = {
            "ms_sort_rows": (i, [vp, i, sz, c_void_pp, u, u, vp, vp, vp]),
            "ms_permute_columns": (i, [vp, i, sz, c_void_pp, c_void_pp, u, vp, sz]),
        }
        # include/ministark_hip_gaps.h: a padded table derived where the trace lies -- select, fill clock gaps, pad
        gap_sigs = {
            "ms_gap_plan": (i, [vp, i, sz, c_void_pp, u, vp, vp, sz, vp, vp]),
            "ms_gap_fill": (i, [vp, i, sz, c_void_pp, u, vp, sz, vp, vp, c_void_pp, u, sz]),
        }
        # include/ministark_hip_join.h: rows joined against a table -- the matched row index, fetched by ms_permute_columns
        join_sigs = {
            "ms_join_rows": (i, [vp, i, sz, c_void_pp, u, vp, sz, c_void_pp, u, u, vp, u, c_void_pp, vp]),
        }
        # include/ministark_hip_range.h: range-check columns -- the limbs of a value column, the multiplicities of the table 0 .. 2^bits - 1
        range_sigs = {
            "ms_limb_decompose": (i, [vp, i, sz, c_void_pp, u, vp, u, vp]),
            "ms_range_multiplicities": (i, [vp, i, sz, c_void_pp, u, u, vp, u, sz, vp, vp]),
        }
        # include/ministark_hip_bitwise.h: bitwise-operation columns -- a op b, the table over limb pairs, its direct-indexed multiplicities
        bitwise_sigs = {
            "ms_bitwise_columns": (i, [vp, i, sz, c_void_pp, u, vp, u, vp]),
            "ms_bitwise_table": (i, [vp, i, u, vp, u, sz, vp, vp, vp, vp]),
            "ms_bitwise_multiplicities": (i, [vp, i, sz, c_void_pp, u, u, vp, u, vp, u, sz, vp, vp]),
        }
        # include/ministark_hip_poseidon.h: Starknet's Poseidon over the 252-bit field -- the bulk permutation and the commitments
        poseidon_sigs = {
            "ms_poseidon252_permute": (i, [vp, sz, vp, vp]),
            "ms_poseidon252_rows": (i, [vp, sz, c_void_pp, u, vp]),
            "ms_poseidon252_rows_row_major": (i, [vp, sz, u, vp, vp]),
            "ms_poseidon252_merkle": (i, [vp, sz, vp, vp]),
        }
        self.optional = {}
        for name, (res, args) in (list(sigs.items()) + list(transcript_sigs.items()) + list(keccak_sigs.items()) + list(ext_sigs.items())
                                  + list(logup_sigs.items()) + list(rpo_coin_sigs.items()) + list(lookup_sigs.items()) + list(sort_sigs.items()) + list(gap_sigs.items())
                                  + list(join_sigs.items()) + list(poseidon_sigs.items()) + list(hades_coin_sigs.items()) + list(blake3_sigs.items()) + list(range_sigs.items()) + list(bitwise_sigs.items())):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        self.sigs = sigs
        self.transcript_sigs = transcript_sigs
        self.keccak_sigs = keccak_sigs
        self.ext_sigs = ext_sigs
        self.logup_sigs = logup_sigs
        self.rpo_coin_sigs = rpo_coin_sigs
        self.lookup_sigs = lookup_sigs
        self.sort_sigs = sort_sigs
        self.gap_sigs = gap_sigs
        self.join_sigs = join_sigs
        self.poseidon_sigs = poseidon_sigs
        self.hades_coin_sigs = hades_coin_sigs
        self.blake3_sigs = blake3_sigs
        self.range_sigs = range_sigs
        self.bitwise_sigs = bitwise_sigs

    def declare(self, name, res, args):
        fn = getattr(self.L, name)
        fn.restype = res
        fn.argtypes = args
        return fn

    def jit_stats(self, handle=None):
        """Specialised constraint kernels of a context (None: of the whole process): compiled / loaded from the disk cache / left to the
        interpreter, and the milliseconds each cost (ms_eval_jit_stats)."""
        st = JitStats()
        self.check(self.L.ms_eval_jit_stats(handle, ctypes.byref(st)))
        return st.as_dict()

    def check(self, rc):
        if rc != 0:
            raise MsError(rc, self.L.ms_last_error().decode())

    def __getattr__(self, name):
        return getattr(self.L, name)


_default = None


def lib():
    global _default
    if _default is None:
        _default = Lib()
    return _default
