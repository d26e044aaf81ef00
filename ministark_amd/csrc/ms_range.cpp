// Range-check columns -- the limbs of a value column and the direct-indexed multiplicities of the table 0 .. 2^bits - 1:
// include/ministark_hip_range.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_range.h"
#include "range_kernels.h"
#include "count_args.h"

static_assert(msrg::MAXSPECS == (int)MS_RANGE_MAX_SPECS && msrg::MAXSETS == (int)MS_RANGE_MAX_SETS, "range_kernels.h and the header disagree");
static_assert(sizeof(ms_limb_spec) == 32 && sizeof(ms_range_set) == 16 && sizeof(ms_limb_report) == 32 && sizeof(msdc::LimbReport) == sizeof(ms_limb_report), "record layouts");
static_assert(sizeof(mslk::Report) == sizeof(ms_lookup_report) && sizeof(msrg::Spec) == 32, "record layouts");
static_assert(MS_RANGE_MAX_LIMB_BITS == 32 && MS_RANGE_MAX_TABLE_BITS == 24, "a limb is a uint32; no bin is mslk::EMPTY");

extern "C" int ms_limb_decompose(ms_ctx* ctx, int field, size_t n, void* const* d_base, unsigned nbase,
                                 const void* h_specs, unsigned nspecs, void* d_report) {
    const char* me = "ms_limb_decompose";
    if (!ctx || !d_base || (nspecs && !h_specs) || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: limbs are columns of a base trace, over Fp or Fp252, not Fq3", me);
    if (nspecs > (unsigned)MS_RANGE_MAX_SPECS) return fail(MS_ERR_INVALID, "%s: %u specs in one call (at most %d)", me, nspecs, MS_RANGE_MAX_SPECS);
    if (n > ((size_t)1 << 32)) return fail(MS_ERR_INVALID, "%s: %zu rows (at most 2^32: the first overflowing row travels as spec << 32 | row)", me, n);
    BaseColumns R(me, (const void* const*)d_base, nbase);             // R.used: the columns that are READ -- sources and masks
    MSCHK(R.null_check());
    const ms_limb_spec* H = (const ms_limb_spec*)h_specs;
    std::vector<msrg::Spec> specs(nspecs);
    std::vector<mscount::Dst> dst(nspecs);
    double bytes = 0;                                                 // the source, the mask, every limb column
    for (unsigned k = 0; k < nspecs; k++) {
        char who[32];
        snprintf(who, sizeof who, "spec %u: ", k);
        const std::string src = std::string(who) + "source ";
        MSCHK(R.col(H[k].src, src.c_str(), &specs[k].src));
        MSCHK(R.mask(H[k].mask, H[k].mask_col, who, &specs[k].mask));
        if (H[k].bits < 1 || H[k].bits > MS_RANGE_MAX_LIMB_BITS) return fail(MS_ERR_INVALID, "%s: %sa limb has 1 .. %d bits, not %d", me, who, MS_RANGE_MAX_LIMB_BITS, H[k].bits);
        if (H[k].nlimbs < 1 || H[k].nlimbs > MS_RANGE_MAX_LIMBS) return fail(MS_ERR_INVALID, "%s: %s1 .. %d limbs, not %d", me, who, MS_RANGE_MAX_LIMBS, H[k].nlimbs);
        if ((unsigned)H[k].nlimbs * (unsigned)H[k].bits > 64 * V)
            return fail(MS_ERR_INVALID, "%s: %s%d limbs of %d bits are more than the %u bits of an element's words", me, who, H[k].nlimbs, H[k].bits, 64 * V);
        if (H[k].dst0 < 0 || (unsigned)H[k].dst0 >= nbase || (unsigned)H[k].nlimbs > nbase - (unsigned)H[k].dst0)
            return fail(MS_ERR_INVALID, "%s: %sdestination columns %d .. %lld out of range (%u)", me, who, H[k].dst0, (long long)H[k].dst0 + H[k].nlimbs - 1, nbase);
        specs[k].dst0 = (uint32_t)H[k].dst0; specs[k].nlimbs = (uint32_t)H[k].nlimbs; specs[k].bits = (uint32_t)H[k].bits; specs[k].mask_kind = H[k].mask;
        dst[k] = {specs[k].dst0, specs[k].dst0 + specs[k].nlimbs};
        bytes += (1.0 + (specs[k].mask ? 1.0 : 0.0) + specs[k].nlimbs) * (double)(n * V * 8);
    }
    // two destination columns clash by index alone, and d_report meets the read columns before the destinations
    static const mscount::Writer<msrg::Spec> W = {"its source or its mask", "limb_clear", "limb_decompose", "limb_finish",
        msrg::limb_decompose<msstage::FpT>, msrg::limb_decompose<msstage::Fp252T>, msrg::limb_finish, false, false};
    return mscount::write_columns(ctx, R, W, field, V, n, d_base, specs, dst, d_report, bytes);
}

template <int V, class F>
static void range_launch(ms_ctx* ctx, const msrg::CountParams& P, bool lds) {
    using namespace msrg;
    const double rows = (double)P.n * P.nsets;
    // each of G workgroups flushes up to 2^bits bins
    auto lds_grid = [&](unsigned cap) { return mscount::lds_grid(P.n, (unsigned long long)P.n * P.nsets, 4ull << P.bits, cap); };
    if (P.n && P.nsets) {
        if (!lds) {
            ProfScope ps(ctx, "range_count_plain", rows * (8.0 * V + 4.0));
            hipLaunchKernelGGL((range_count_plain<V>), dim3(stream_grid(P.n), P.nsets), dim3(NT), 0, ctx->stream, P);
        } else {
            ProfScope ps(ctx, "range_count_lds", rows * 8.0 * V);
            // 16 KiB histograms: two workgroups of 1024 lanes fill a CU's 32 wave slots; 128 KiB ones: one per CU
            if (P.bits <= 12) hipLaunchKernelGGL((range_count_lds<V, 12>), dim3(lds_grid(512)), dim3(LNT), 0, ctx->stream, P);
            else if (P.bits <= 15) hipLaunchKernelGGL((range_count_lds<V, 15>), dim3(lds_grid(256)), dim3(LNT), 0, ctx->stream, P);
            else hipLaunchKernelGGL((range_count_lds<V, 16>), dim3(lds_grid(256)), dim3(LNT), 0, ctx->stream, P);
        }
    }
    { ProfScope ps(ctx, "range_finish", 4.0 * (double)((size_t)1 << P.bits) + 8.0 * V * (double)P.n_m);
      hipLaunchKernelGGL((range_finish<F>), dim3(stream_grid(P.n_m)), dim3(NT), 0, ctx->stream, P); }
}

extern "C" int ms_range_multiplicities(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned bits,
                                       const void* h_sets, unsigned nsets, size_t n_m, void* d_m, void* d_report) {
    const char* me = "ms_range_multiplicities";
    if (!ctx || !d_base || (nsets && !h_sets) || !d_m || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: looked-up columns are columns of a base trace, over Fp or Fp252, not Fq3", me);
    if (bits < 1 || bits > (unsigned)MS_RANGE_MAX_TABLE_BITS) return fail(MS_ERR_INVALID, "%s: a table of 2^bits rows has bits in 1 .. %d, not %u", me, MS_RANGE_MAX_TABLE_BITS, bits);
    if (nsets > (unsigned)MS_RANGE_MAX_SETS) return fail(MS_ERR_UNSUPPORTED, "%s: %u lookup sets in one call (at most %d)", me, nsets, MS_RANGE_MAX_SETS);
    if (n_m < ((size_t)1 << bits)) return fail(MS_ERR_INVALID, "%s: d_m holds %zu elements, fewer than the 2^%u rows of the table", me, n_m, bits);
    BaseColumns R(me, d_base, nbase);                                 // R.used: the base columns a set or a mask names
    MSCHK(R.null_check());
    msrg::CountParams P;
    memset(&P, 0, sizeof P);
    for (unsigned s = 0; s < nsets; s++) {
        const ms_range_set& H = ((const ms_range_set*)h_sets)[s];
        char who[32];
        snprintf(who, sizeof who, "lookup set %u: ", s);
        MSCHK(R.col(H.col, who, &P.sets[s].col));
        MSCHK(R.mask(H.mask, H.mask_col, who, &P.sets[s].mask));
        P.sets[s].mask_kind = H.mask;
    }
    if (n > ((size_t)1 << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu rows (at most 2^32: the first missing row travels as set << 32 | row)", me, n);
    if ((unsigned long long)nsets * n >= (1ull << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %u sets of %zu rows (the counters are 32-bit: sets * rows < 2^32)", me, nsets, n);
    P.bits = bits; P.nsets = nsets;
    return mscount::count_scratch(ctx, R, field, V, n, n_m, d_m, d_report, "MS_RANGE_FORM", bits <= 16, (size_t)1 << bits, "range_clear", P, [&](bool lds) {
        if (V == 1) range_launch<1, msstage::FpT>(ctx, P, lds);
        else range_launch<4, msstage::Fp252T>(ctx, P, lds);
    });
}
