// Bitwise-operation columns -- a op b as a base column, the table (op, x, y, x op y) over limb pairs and its direct-indexed
// multiplicities: include/ministark_hip_bitwise.h.
#include "ms_internal.h"
#include "../../include/ministark_hip_bitwise.h"
#include "bitwise_kernels.h"
#include "count_args.h"

static_assert(msbw::MAXSPECS == (int)MS_BITWISE_MAX_SPECS && msbw::MAXSETS == (int)MS_BITWISE_MAX_SETS && msbw::MAXOPS == (int)MS_BITWISE_MAX_OPS, "bitwise_kernels.h and the header disagree");
static_assert(msbw::OP_AND == (int)MS_BIT_AND && msbw::OP_OR == (int)MS_BIT_OR && msbw::OP_XOR == (int)MS_BIT_XOR, "op codes");
static_assert(sizeof(ms_bitwise_spec) == 32 && sizeof(ms_bitwise_set) == 32 && sizeof(msbw::Spec) == 40 && sizeof(msdc::LimbReport) == sizeof(ms_limb_report), "record layouts");
static_assert(sizeof(msbw::CountParams) <= 3584, "the sets travel as a kernel argument");
static_assert(MS_BITWISE_MAX_BITS == 12 && MS_BITWISE_MAX_TABLE_LOG == 24, "a bin is a uint32 below mslk::EMPTY; a limb pair is 24 bits");
static_assert(2 * msbw::PACKED_BITS == 16, "the packed histogram has 2^16 bins");

// 2^wmax is the widest power of two below the modulus: the OR or XOR of two operands below it is canonical
static unsigned wmax_of(unsigned V) { return V == 1 ? 63u : 251u; }

static int check_op(const char* me, const char* who, int op) {
    if (op != MS_BIT_AND && op != MS_BIT_OR && op != MS_BIT_XOR) return fail(MS_ERR_INVALID, "%s: %sunknown op %d (MS_BIT_AND, MS_BIT_OR, MS_BIT_XOR)", me, who, op);
    return MS_OK;
}

// bits, the ops and T = nops * 4^bits of a table; *T is at most 2^24
static int check_table(const char* me, unsigned bits, const int32_t* h_ops, unsigned nops, size_t* T) {
    if (bits < 1 || bits > (unsigned)MS_BITWISE_MAX_BITS) return fail(MS_ERR_INVALID, "%s: a limb has 1 .. %d bits, not %u", me, MS_BITWISE_MAX_BITS, bits);
    if (nops < 1 || nops > (unsigned)MS_BITWISE_MAX_OPS) return fail(MS_ERR_INVALID, "%s: 1 .. %d ops, not %u", me, MS_BITWISE_MAX_OPS, nops);
    for (unsigned s = 0; s < nops; s++) {
        MSCHK(check_op(me, "", h_ops[s]));
        for (unsigned t = 0; t < s; t++)
            if (h_ops[t] == h_ops[s]) return fail(MS_ERR_INVALID, "%s: op %d is named twice", me, h_ops[s]);
    }
    *T = (size_t)nops << (2 * bits);
    if (*T > ((size_t)1 << MS_BITWISE_MAX_TABLE_LOG)) return fail(MS_ERR_INVALID, "%s: %u ops over pairs of %u-bit limbs are %zu table rows (at most 2^%d)", me, nops, bits, *T, MS_BITWISE_MAX_TABLE_LOG);
    return MS_OK;
}

extern "C" int ms_bitwise_columns(ms_ctx* ctx, int field, size_t n, void* const* d_base, unsigned nbase,
                                  const void* h_specs, unsigned nspecs, void* d_report) {
    const char* me = "ms_bitwise_columns";
    if (!ctx || !d_base || (nspecs && !h_specs) || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: operands are columns of a base trace, over Fp or Fp252, not Fq3", me);
    if (nspecs > (unsigned)MS_BITWISE_MAX_SPECS) return fail(MS_ERR_INVALID, "%s: %u specs in one call (at most %d)", me, nspecs, MS_BITWISE_MAX_SPECS);
    if (n > ((size_t)1 << 32)) return fail(MS_ERR_INVALID, "%s: %zu rows (at most 2^32: the first overflowing row travels as spec << 32 | row)", me, n);
    BaseColumns R(me, (const void* const*)d_base, nbase);             // R.used: the columns that are READ -- operands and masks
    MSCHK(R.null_check());
    const ms_bitwise_spec* H = (const ms_bitwise_spec*)h_specs;
    std::vector<msbw::Spec> specs(nspecs);
    std::vector<mscount::Dst> dst(nspecs);
    double bytes = 0;                                                 // the operands (once when a == b), the mask, the result
    for (unsigned k = 0; k < nspecs; k++) {
        char who[32];
        snprintf(who, sizeof who, "spec %u: ", k);
        const std::string opa = std::string(who) + "operand a ", opb = std::string(who) + "operand b ";
        MSCHK(check_op(me, who, H[k].op));
        MSCHK(R.col(H[k].a, opa.c_str(), &specs[k].a));
        MSCHK(R.col(H[k].b, opb.c_str(), &specs[k].b));
        MSCHK(R.mask(H[k].mask, H[k].mask_col, who, &specs[k].mask));
        if (H[k].width < 1 || (unsigned)H[k].width > wmax_of(V)) return fail(MS_ERR_INVALID, "%s: %san operand has 1 .. %u bits, not %d", me, who, wmax_of(V), H[k].width);
        if (H[k].dst < 0 || (unsigned)H[k].dst >= nbase) return fail(MS_ERR_INVALID, "%s: %sdestination column %d out of range (%u)", me, who, H[k].dst, nbase);
        specs[k].dst = (uint32_t)H[k].dst; specs[k].width = (uint32_t)H[k].width; specs[k].op = (uint32_t)H[k].op; specs[k].mask_kind = H[k].mask;
        dst[k] = {specs[k].dst, specs[k].dst + 1};
        bytes += ((specs[k].a == specs[k].b ? 1.0 : 2.0) + (specs[k].mask ? 1.0 : 0.0) + 1.0) * (double)(n * V * 8);
    }
    // two destination columns clash by address too, and d_report meets a spec's destination before the next spec is looked at
    static const mscount::Writer<msbw::Spec> W = {"an operand or its mask", "bitwise_clear", "bitwise_columns", "bitwise_col_finish",
        msbw::bitwise_columns<msstage::FpT>, msbw::bitwise_columns<msstage::Fp252T>, msbw::bitwise_col_finish, true, true};
    return mscount::write_columns(ctx, R, W, field, V, n, d_base, specs, dst, d_report, bytes);
}

extern "C" int ms_bitwise_table(ms_ctx* ctx, int field, unsigned bits, const void* h_op_codes, unsigned nops, size_t n_t,
                                void* d_top, void* d_tx, void* d_ty, void* d_tz) {
    const char* me = "ms_bitwise_table";
    const int32_t* h_ops = (const int32_t*)h_op_codes;
    if (!ctx || !h_ops || !d_tx || !d_ty || !d_tz) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: the table's columns are columns of a base trace, over Fp or Fp252, not Fq3", me);
    size_t T = 0;
    MSCHK(check_table(me, bits, h_ops, nops, &T));
    if (n_t < T) return fail(MS_ERR_INVALID, "%s: the columns hold %zu elements, fewer than the %zu rows of the table", me, n_t, T);
    void* outs[4] = {d_tx, d_ty, d_tz, d_top};
    const char* names[4] = {"d_tx", "d_ty", "d_tz", "d_top"};
    const size_t col_bytes = n_t * V * 8;
    for (int x = 0; x < 4; x++)
        for (int y = 0; y < x; y++)
            if (outs[x] && outs[y] && ranges_overlap(outs[x], col_bytes, outs[y], col_bytes)) return fail(MS_ERR_INVALID, "%s: %s and %s overlap", me, names[y], names[x]);
    msbw::TableParams P;
    memset(&P, 0, sizeof P);
    P.top = (uint64_t*)d_top; P.tx = (uint64_t*)d_tx; P.ty = (uint64_t*)d_ty; P.tz = (uint64_t*)d_tz;
    P.n_t = n_t; P.T = T; P.bits = bits;
    for (unsigned s = 0; s < nops; s++) P.ops[s] = (unsigned)h_ops[s];
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    { ProfScope ps(ctx, "bitwise_table", (d_top ? 4.0 : 3.0) * (double)col_bytes);
      if (V == 1) hipLaunchKernelGGL((msbw::bitwise_table<msstage::FpT>), dim3(stream_grid(n_t)), dim3(msbw::NT), 0, ctx->stream, P);
      else hipLaunchKernelGGL((msbw::bitwise_table<msstage::Fp252T>), dim3(stream_grid(n_t)), dim3(msbw::NT), 0, ctx->stream, P); }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

template <int V, class F>
static void bitwise_launch(ms_ctx* ctx, const msbw::CountParams& P, unsigned nops, unsigned long long incs, bool lds) {
    using namespace msbw;
    const double rows = (double)P.n * P.nsets;
    // per op slot: each of G workgroups on each of nops slots flushes up to 4^bits bins, and `cap` workgroups in all
    auto lds_grid = [&](unsigned cap) { return mscount::lds_grid(P.n, incs, ((unsigned long long)nops * 4ull) << (2 * P.bits), cap / nops); };
    if (P.n && P.nsets) {
        if (!lds) {
            ProfScope ps(ctx, "bitwise_count_plain", rows * 24.0 * V + 4.0 * (double)incs);
            hipLaunchKernelGGL((bitwise_count_plain<V>), dim3(stream_grid(P.n), P.nsets), dim3(NT), 0, ctx->stream, P);
        } else {
            ProfScope ps(ctx, "bitwise_count_lds", rows * 24.0 * V);
            // 16 KiB histograms: two workgroups of 1024 lanes fill a CU's 32 wave slots; 64 and 128 KiB ones: one per CU
            if (P.bits <= 6) hipLaunchKernelGGL((bitwise_count_lds<V, 12>), dim3(lds_grid(512), nops), dim3(LNT), 0, ctx->stream, P);
            else if (P.bits == 7) hipLaunchKernelGGL((bitwise_count_lds<V, 14>), dim3(lds_grid(256), nops), dim3(LNT), 0, ctx->stream, P);
            else hipLaunchKernelGGL((bitwise_count_lds<V, 16>), dim3(lds_grid(256), nops), dim3(LNT), 0, ctx->stream, P);
        }
    }
    { ProfScope ps(ctx, "bitwise_finish", 4.0 * (double)P.T + 8.0 * V * (double)P.n_m);
      hipLaunchKernelGGL((bitwise_finish<F>), dim3(stream_grid(P.n_m)), dim3(NT), 0, ctx->stream, P); }
}

extern "C" int ms_bitwise_multiplicities(ms_ctx* ctx, int field, size_t n, const void* const* d_base, unsigned nbase, unsigned bits,
                                         const void* h_op_codes, unsigned nops, const void* h_sets, unsigned nsets, size_t n_m, void* d_m, void* d_report) {
    const char* me = "ms_bitwise_multiplicities";
    const int32_t* h_ops = (const int32_t*)h_op_codes;
    if (!ctx || !d_base || !h_ops || (nsets && !h_sets) || !d_m || !d_report) return fail(MS_ERR_INVALID, "%s: null argument", me);
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (V == 3) return fail(MS_ERR_UNSUPPORTED, "%s: looked-up columns are columns of a base trace, over Fp or Fp252, not Fq3", me);
    size_t T = 0;
    MSCHK(check_table(me, bits, h_ops, nops, &T));
    if (nsets > (unsigned)MS_BITWISE_MAX_SETS) return fail(MS_ERR_UNSUPPORTED, "%s: %u lookup sets in one call (at most %d)", me, nsets, MS_BITWISE_MAX_SETS);
    if (n_m < T) return fail(MS_ERR_INVALID, "%s: d_m holds %zu elements, fewer than the %zu rows of the table", me, n_m, T);
    BaseColumns R(me, d_base, nbase);                                 // R.used: the base columns a set or a mask names
    MSCHK(R.null_check());
    msbw::CountParams P;
    memset(&P, 0, sizeof P);
    unsigned long long limbs = 0;
    for (unsigned s = 0; s < nsets; s++) {
        const ms_bitwise_set& H = ((const ms_bitwise_set*)h_sets)[s];
        char who[32];
        snprintf(who, sizeof who, "lookup set %u: ", s);
        const std::string opa = std::string(who) + "operand a ", opb = std::string(who) + "operand b ", res = std::string(who) + "result ";
        MSCHK(check_op(me, who, H.op));
        unsigned slot = 0;
        while (slot < nops && h_ops[slot] != H.op) slot++;
        if (slot == nops) return fail(MS_ERR_INVALID, "%s: %sop %d is not one of the table's ops", me, who, H.op);
        MSCHK(R.col(H.a, opa.c_str(), &P.sets[s].a));
        MSCHK(R.col(H.b, opb.c_str(), &P.sets[s].b));
        if (H.c < -1) return fail(MS_ERR_INVALID, "%s: %sresult column %d (a column index, or -1 for none)", me, who, H.c);
        if (H.c >= 0) MSCHK(R.col(H.c, res.c_str(), &P.sets[s].c));
        MSCHK(R.mask(H.mask, H.mask_col, who, &P.sets[s].mask));
        if (H.nlimbs < 1 || H.nlimbs > MS_BITWISE_MAX_LIMBS) return fail(MS_ERR_INVALID, "%s: %s1 .. %d limbs, not %d", me, who, MS_BITWISE_MAX_LIMBS, H.nlimbs);
        if ((unsigned)H.nlimbs * bits > wmax_of(V))
            return fail(MS_ERR_INVALID, "%s: %s%d limbs of %u bits are more than the %u bits an operand may have", me, who, H.nlimbs, bits, wmax_of(V));
        P.sets[s].mask_kind = H.mask; P.sets[s].op = (uint32_t)H.op; P.sets[s].slot = slot; P.sets[s].nlimbs = (uint32_t)H.nlimbs;
        limbs += (unsigned)H.nlimbs;
        P.max_limbs = std::max(P.max_limbs, (unsigned)H.nlimbs);
    }
    if (n > ((size_t)1 << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %zu rows (at most 2^32: the first missing row travels as set << 32 | row)", me, n);
    const unsigned long long incs = limbs * (unsigned long long)n;   // limbs <= 2^14, n <= 2^32: no wrap
    if (incs >= (1ull << 32)) return fail(MS_ERR_UNSUPPORTED, "%s: %llu limbs a row over %zu rows (the counters are 32-bit: the limb pairs of a call are fewer than 2^32)", me, limbs, n);
    P.T = T; P.bits = bits; P.nsets = nsets;
    // above 2^16 bins an op there is the global form alone
    return mscount::count_scratch(ctx, R, field, V, n, n_m, d_m, d_report, "MS_BITWISE_FORM", bits <= (unsigned)msbw::PACKED_BITS, T, "bitwise_clear", P, [&](bool lds) {
        if (V == 1) bitwise_launch<1, msstage::FpT>(ctx, P, nops, incs, lds);
        else bitwise_launch<4, msstage::Fp252T>(ctx, P, nops, incs, lds);
    });
}
