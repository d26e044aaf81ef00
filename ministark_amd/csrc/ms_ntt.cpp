// NTT / iNTT passes of the Goldilocks fields, the two-pass coset LDE, bit reversal, the fused LDE and evaluate entry points (GpuFft / GpuIfft /
// Matrix methods: gpu/src/plan.rs:186-462, src/matrix.rs:102-251).  The plans and their tables are built in ms_ntt_plan.cpp, the 252-bit
// field's passes run in ms_ntt252.cpp.
#include "ms_internal.h"
#include "ntt2_kernels.h"
#include "lde2_kernels.h"
#include "stage_kernels.h"
#include "scan_kernels.h"

// The column chains' defaults (profiles/ntt_column_chains.txt): on or off, streams, smallest column (log2 points)
static constexpr bool CHAIN_DEFAULT_ON = true;
static constexpr unsigned CHAIN_STREAMS = 2, CHAIN_MIN_LOG = 23;
// The switches read once per process, at the first transform.
struct NttSwitches {
    // MS_NTT_FUSED_SMALL=0: 2^11 .. 2^14-point Fp columns take the launches they took before ntt_fused_tiny / ntt_fused_small (before / after timings)
    bool fused_off = getenv("MS_NTT_FUSED_SMALL") && !strcmp(getenv("MS_NTT_FUSED_SMALL"), "0");
    // MS_NTT_FUSED_MAX_LOG: the largest size (log2) that takes ntt_fused_small, at most 14
    unsigned fused_max = getenv("MS_NTT_FUSED_MAX_LOG") ? (unsigned)atoi(getenv("MS_NTT_FUSED_MAX_LOG")) : 14u;
    // MS_NTT_INV18_TWO_PASS=0: inverse transforms of 2^18 points on the three passes
    bool inv18_off = getenv("MS_NTT_INV18_TWO_PASS") && !strcmp(getenv("MS_NTT_INV18_TWO_PASS"), "0");
    // MS_NTT_STREAMS=2: the two halves of a group on two streams -- kernels of different passes then overlap (a pass
    // alternates between a memory phase and an arithmetic phase per workgroup); measured 162 -> 159 us per 2^24 column
    // over 8 columns.  Off by default: with concurrent kernels the per-kernel durations of a trace no longer add up to the
    // wall time, and the gain is under 2 %.  Never while per-launch profiling is on (its events sit on one stream).
    // Columns below 2^20 points lose with it (round 4, MS_NTT_STREAMS_MIN_LOG=12: 2^16 x 128 0.67 -> 0.88 us per column, 2^17 x 64 1.40 -> 1.60).
    bool two_streams = getenv("MS_NTT_STREAMS") != nullptr && atoi(getenv("MS_NTT_STREAMS")) == 2;
    unsigned two_min_log = getenv("MS_NTT_STREAMS_MIN_LOG") ? (unsigned)atoi(getenv("MS_NTT_STREAMS_MIN_LOG")) : 20u;
    // MS_NTT_CHAINS: the column chains of run_passes (CHAIN_DEFAULT_ON decides without it: =0 the batch launches, =1 the chains);
    // MS_NTT_CHAIN_STREAMS (1 .. 4, never more: the runtime's queue limit) and MS_NTT_CHAIN_MIN_LOG override the number of streams and the
    // smallest column (log2 points) that takes the route -- for measurements and tests
    bool chains = getenv("MS_NTT_CHAINS") ? !strcmp(getenv("MS_NTT_CHAINS"), "1") : CHAIN_DEFAULT_ON;
    unsigned chain_streams = getenv("MS_NTT_CHAIN_STREAMS") ? (unsigned)std::min(std::max(atoi(getenv("MS_NTT_CHAIN_STREAMS")), 1), MAX_CHAINS) : CHAIN_STREAMS;
    unsigned chain_min_log = getenv("MS_NTT_CHAIN_MIN_LOG") ? (unsigned)atoi(getenv("MS_NTT_CHAIN_MIN_LOG")) : CHAIN_MIN_LOG;
    // MS_LDE2_FQ3=0: Fq3 columns off the two-pass coset LDE (before / after timings, tests of the three-pass route); =all: from 2^17 rows
    // on (the tests reach the T = 2 instantiation)
    bool fq3_off = getenv("MS_LDE2_FQ3") && !strcmp(getenv("MS_LDE2_FQ3"), "0");
    bool fq3_all = getenv("MS_LDE2_FQ3") && !strcmp(getenv("MS_LDE2_FQ3"), "all");
    // MS_NTT_DEBUG: one line per pass of the pass loop on stderr (the 252-bit tiled path reads it per call: ms_ntt252.cpp)
    bool debug = getenv("MS_NTT_DEBUG") != nullptr;
};
static const NttSwitches& switches() { static const NttSwitches s{}; return s; }

// non-temporal tile accesses once the columns of a launch and their scratch exceed the Infinity Cache (ntt2_kernels.h): STREAM of the limb-form kernels
static bool beyond_cache(unsigned nc, size_t col_bytes) { return 2 * (size_t)nc * col_bytes > ((size_t)256 << 20); }

// ---------------------------------------------------------------------------------------
// kernel choice: every picker names exactly the instantiations the library holds
// ---------------------------------------------------------------------------------------
using KFused = void (*)(msntt::FusedParams);
using K1 = void (*)(msntt::PassParams);
using K2 = void (*)(msntt2::Params);
using KLde = void (*)(mslde2::Params);

static KFused fused_tiny_kernel(const ms_ntt_plan* p) {
    using namespace msntt;
    if (p->inverse) return p->scale_mode == 2 ? ntt_fused_tiny<11, true, false, 2> : p->scale_mode == 1 ? ntt_fused_tiny<11, true, false, 1> : ntt_fused_tiny<11, true, false, 0>;
    return p->coset ? ntt_fused_tiny<11, false, true, 0> : ntt_fused_tiny<11, false, false, 0>;
}
template <int LOGN> static KFused fused_small_kernel(const ms_ntt_plan* p) {
    using namespace msntt;
    if (p->inverse) return p->scale_mode == 2 ? ntt_fused_small<LOGN, true, false, 2> : p->scale_mode == 1 ? ntt_fused_small<LOGN, true, false, 1> : ntt_fused_small<LOGN, true, false, 0>;
    return p->coset ? ntt_fused_small<LOGN, false, true, 0> : ntt_fused_small<LOGN, false, false, 0>;
}
static KFused fused_small_kernel(const ms_ntt_plan* p) {
    return p->log_n == 12 ? fused_small_kernel<12>(p) : p->log_n == 13 ? fused_small_kernel<13>(p) : fused_small_kernel<14>(p);
}

// round-1 passes (ntt_kernels.h).  na: sixteenths of the first pass's rows that hold data (16: all of them)
template <bool COS> static K1 first_pass_r1(int na) {
    using namespace msntt;
    return na == 4 ? ntt_first_pass<false, COS, 4> : na == 2 ? ntt_first_pass<false, COS, 2> : na == 1 ? ntt_first_pass<false, COS, 1> : ntt_first_pass<false, COS>;
}
static K1 first_pass_r1(bool inverse, bool coset, int na) {
    if (inverse) return msntt::ntt_first_pass<true, false>;
    return coset ? first_pass_r1<true>(na) : first_pass_r1<false>(na);
}
template <int RB, bool INV> static K1 mid_pass_r1(bool last, int scale, bool bitrev) {
    using namespace msntt;
    if (!last) return ntt_mid_pass<RB, INV, false, 0>;
    if (bitrev)        // fused bit-reversed store (LDE): forward transforms only carry scale 0
        return scale == 1 ? ntt_mid_pass<RB, INV, true, 1, true> : scale == 2 ? ntt_mid_pass<RB, INV, true, 2, true> : ntt_mid_pass<RB, INV, true, 0, true>;
    return scale == 1 ? ntt_mid_pass<RB, INV, true, 1> : scale == 2 ? ntt_mid_pass<RB, INV, true, 2> : ntt_mid_pass<RB, INV, true, 0>;
}
template <int RB> static K1 mid_pass_r1(bool inverse, bool last, int scale, bool bitrev) {
    return inverse ? mid_pass_r1<RB, true>(last, scale, bitrev) : mid_pass_r1<RB, false>(last, scale, bitrev);
}
// log_r: the pass's radix, 2^4 .. 2^8 (null otherwise); scale: the plan's scale_mode, applied by the last pass
static K1 mid_pass_r1(unsigned log_r, bool inverse, bool last, int scale, bool bitrev) {
    switch (log_r) {
    case 4: return mid_pass_r1<1>(inverse, last, scale, bitrev);
    case 5: return mid_pass_r1<2>(inverse, last, scale, bitrev);
    case 6: return mid_pass_r1<4>(inverse, last, scale, bitrev);
    case 7: return mid_pass_r1<8>(inverse, last, scale, bitrev);
    case 8: return mid_pass_r1<16>(inverse, last, scale, bitrev);
    default: return nullptr;
    }
}

// limb-form passes (ntt2_kernels.h), S = STREAM.  First pass: an inverse transform has neither the coset factor nor pruned rows;
// (UNI, PERM) is (t, t) for Fp columns of a uniform-factor plan, (t, f) for its Fq3 columns, (f, f) otherwise
template <bool S, bool INV, bool COS, int NA> static K2 first_pass_layout(bool uni, bool perm) {
    using namespace msntt2;
    return perm ? ntt2_first_pass<S, INV, COS, NA, true, true> : uni ? ntt2_first_pass<S, INV, COS, NA, true> : ntt2_first_pass<S, INV, COS, NA, false>;
}
template <bool S, bool COS> static K2 first_pass_rows(int na, bool uni, bool perm) {
    return na == 4 ? first_pass_layout<S, false, COS, 4>(uni, perm) : na == 2 ? first_pass_layout<S, false, COS, 2>(uni, perm)
         : na == 1 ? first_pass_layout<S, false, COS, 1>(uni, perm) : first_pass_layout<S, false, COS, 16>(uni, perm);
}
template <bool S> static K2 first_pass_kernel(bool inverse, bool coset, int na, bool uni, bool perm) {
    if (inverse) return first_pass_layout<S, true, false, 16>(uni, perm);
    return coset ? first_pass_rows<S, true>(na, uni, perm) : first_pass_rows<S, false>(na, uni, perm);
}
// the middle pass of a (256, R, 256) plan, R = 2^log_r < 256: R <= 16 holds its whole network in registers
template <bool S, bool INV, bool PERM> static K2 small_mid_kernel(unsigned log_r) {
    using namespace msntt2;
    switch (log_r) {
    case 1: return ntt2_small_mid_pass<S, INV, 1, PERM>;
    case 2: return ntt2_small_mid_pass<S, INV, 2, PERM>;
    case 3: return ntt2_small_mid_pass<S, INV, 3, PERM>;
    case 4: return ntt2_small_mid_pass<S, INV, 4, PERM>;
    case 5: return ntt2_mid_pass_r<S, INV, 1, PERM>;
    case 6: return ntt2_mid_pass_r<S, INV, 2, PERM>;
    default: return ntt2_mid_pass_r<S, INV, 3, PERM>;
    }
}
template <bool S> static K2 small_mid_kernel(unsigned log_r, bool inverse, bool perm) {
    if (inverse) return perm ? small_mid_kernel<S, true, true>(log_r) : small_mid_kernel<S, true, false>(log_r);
    return perm ? small_mid_kernel<S, false, true>(log_r) : small_mid_kernel<S, false, false>(log_r);
}
// a radix-256 pass after the first.  Not last: with PERM it reads pass 1's permuted rows and writes the natural order (in place); in a uniform-factor
// plan it applies the per-lane remainder of pass 1's factor on its loads.  Last: the scale modes exist for the inverse only.
template <bool S, bool INV> static K2 mid_pass_kernel(bool uni, bool perm) {
    using namespace msntt2;
    return perm ? ntt2_mid_pass<S, INV, false, 0, true, true> : uni ? ntt2_mid_pass<S, INV, false, 0, true> : ntt2_mid_pass<S, INV, false, 0>;
}
template <bool S> static K2 last_pass_kernel(bool inverse, int scale, bool bitrev) {
    using namespace msntt2;
    if (bitrev) return ntt2_last_pass_bitrev<S>;
    if (!inverse) return ntt2_mid_pass<S, false, true, 0>;
    return scale == 2 ? ntt2_mid_pass<S, true, true, 2> : scale == 1 ? ntt2_mid_pass<S, true, true, 1> : ntt2_mid_pass<S, true, true, 0>;
}
// pass q of the plan as a limb-form kernel
template <bool S> static K2 limb_pass_kernel(const ms_ntt_plan* p, int q, int na, bool small_mid, bool perm, bool bitrev_out) {
    if (q == 0) return first_pass_kernel<S>(p->inverse, !p->inverse && p->coset, na, p->uni, perm);
    if (small_mid) return small_mid_kernel<S>(p->lr[q], p->inverse, perm);
    if (q < p->npass - 1) return p->inverse ? mid_pass_kernel<S, true>(p->uni, perm) : mid_pass_kernel<S, false>(p->uni, perm);
    return last_pass_kernel<S>(p->inverse, p->scale_mode, bitrev_out);
}

// ... under cache policy `pol` (ntt2_kernels.h).  Both sides hinted or neither: every pass of every limb-form plan (the batch launches).  One side:
// what the column chains launch -- loads-only the first pass, stores-only the last natural-order pass, of Fp columns of a uniform-factor plan
static K2 limb_pass_kernel(int pol, const ms_ntt_plan* p, int q, int na, bool small_mid, bool perm, bool bitrev_out) {
    using namespace msntt2;
    switch (pol) {
    case POL_PLAIN: return limb_pass_kernel<false>(p, q, na, small_mid, perm, bitrev_out);
    case POL_NT: return limb_pass_kernel<true>(p, q, na, small_mid, perm, bitrev_out);
    case POL_NT_LD:
        if (q != 0 || !perm || na != 16) return nullptr;
        if (p->inverse) return ntt2_first_pass<true, true, false, 16, true, true, POL_NT_LD>;
        return p->coset ? ntt2_first_pass<true, false, true, 16, true, true, POL_NT_LD> : ntt2_first_pass<true, false, false, 16, true, true, POL_NT_LD>;
    case POL_NT_ST:
        if (q != p->npass - 1 || q == 0 || small_mid || bitrev_out) return nullptr;
        if (!p->inverse) return ntt2_mid_pass<true, false, true, 0, false, false, POL_NT_ST>;
        return p->scale_mode == 2 ? ntt2_mid_pass<true, true, true, 2, false, false, POL_NT_ST>
             : p->scale_mode == 1 ? ntt2_mid_pass<true, true, true, 1, false, false, POL_NT_ST> : ntt2_mid_pass<true, true, true, 0, false, false, POL_NT_ST>;
    default: return nullptr;
    }
}

// the two-pass coset LDE (lde2_kernels.h).  Pass A: Fq3 columns (V = 3) without the uniform split (T = 2) have the streaming variant alone;
// rev: the column backwards, an inverse transform's pass A (Fp, uniform split)
static KLde lde2_pass_a_kernel(bool stream, bool uni, unsigned V, bool rev) {
    using namespace mslde2;
    if (V == 3) return !uni ? lde2_strided_pass<true, false, 3> : stream ? lde2_strided_pass<true, true, 3> : lde2_strided_pass<false, true, 3>;
    if (rev) return stream ? lde2_strided_pass<true, true, 1, true> : lde2_strided_pass<false, true, 1, true>;
    if (stream) return uni ? lde2_strided_pass<true, true> : lde2_strided_pass<true, false>;
    return uni ? lde2_strided_pass<false, true> : lde2_strided_pass<false, false>;
}
// Pass B, T = n / 2^16.  natural: the 2^18-point transform in natural order (T = 4), oscale 0 / 1 / 2 = none / the constant / the table of an inverse
template <bool S> static KLde lde2_pass_b_kernel(unsigned T, bool uni, unsigned V, bool natural, int oscale) {
    using namespace mslde2;
    if (V == 3)
        switch (T) {
        case 16: return lde2_rows_pass<S, 16, true, false, 3>;
        case 8: return lde2_rows_pass<S, 8, true, false, 3>;
        case 4: return lde2_rows_pass<S, 4, true, false, 3>;
        default: return lde2_rows_pass<S, 2, false, false, 3>;
        }
    if (natural) return oscale == 2 ? lde2_rows_pass<S, 4, true, true, 1, 2> : oscale == 1 ? lde2_rows_pass<S, 4, true, true, 1, 1> : lde2_rows_pass<S, 4, true, true>;
    switch (T) {
    case 64: return lde2_rows_pass<S, 64, true>;
    case 32: return lde2_rows_pass<S, 32, true>;
    case 16: return uni ? lde2_rows_pass<S, 16, true> : lde2_rows_pass<S, 16, false>;
    case 8: return uni ? lde2_rows_pass<S, 8, true> : lde2_rows_pass<S, 8, false>;
    case 4: return uni ? lde2_rows_pass<S, 4, true> : lde2_rows_pass<S, 4, false>;
    default: return lde2_rows_pass<S, 2, false>;
    }
}

// ---------------------------------------------------------------------------------------
// the routes of a Goldilocks transform
// ---------------------------------------------------------------------------------------
// The column pointers of the one-launch kernels travel as a table {src, dst} per column, read in place from the staging ring (stage_view):
// hands the staged table and its column count to `launch`, 4096 columns (64 KiB of pointers: an eighth of the ring's half) at a time.
template <class Launch>
static int with_column_tables(ms_ctx* ctx, const void* const* src, void* const* dst, unsigned ncols, Launch&& launch) {
    constexpr unsigned PER_LAUNCH = 4096;
    for (unsigned c0 = 0; c0 < ncols; c0 += PER_LAUNCH) {
        const unsigned nc = std::min<unsigned>(PER_LAUNCH, ncols - c0);
        std::vector<const void*> tab(2 * (size_t)nc);
        for (unsigned c = 0; c < nc; c++) { tab[2 * c] = src[c0 + c]; tab[2 * c + 1] = dst[c0 + c]; }
        LockedPoolGuard pooled(ctx);
        const void* d_tab = nullptr;
        MSCHK(stage_view(ctx, tab.data(), tab.size() * sizeof(void*), &d_tab, pooled));
        launch((const uint64_t* const*)d_tab, nc);
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// log_n < 12: one workgroup per column (ntt_small)
static int run_small(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols) {
    ms_ctx* ctx = p->ctx;
    const size_t col_bytes = ((size_t)1 << p->log_n) * p->V * 8;
    return with_column_tables(ctx, src, dst, ncols, [&](const uint64_t* const* d_tab, unsigned nc) {
        msntt::SmallParams S;
        memset(&S, 0, sizeof S);
        S.cols = d_tab;
        S.tw = p->d_tw; S.scale_in = p->d_scale_in; S.scale_out = p->d_scale_out; S.log_n = p->log_n; S.V = p->V;
        ProfScope ps(ctx, "ntt_small", 2.0 * col_bytes * nc);
        hipLaunchKernelGGL(msntt::ntt_small, dim3(1, nc), dim3(msntt::NT), 0, ctx->stream, S);
    });
}

// 2^11-point Fp columns (ntt_fused_tiny: two columns per workgroup) and 2^12 .. 2^14-point ones (ntt_fused_small: the (256, 16) .. (256, 64) plans):
// both passes in ONE launch, the column stays in LDS in between, and one launch takes any number of columns
static int run_fused(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols) {
    ms_ctx* ctx = p->ctx;
    const size_t col_bytes = ((size_t)1 << p->log_n) * 8;
    const bool tiny = p->small;
    const KFused k = tiny ? fused_tiny_kernel(p) : fused_small_kernel(p);
    return with_column_tables(ctx, src, dst, ncols, [&](const uint64_t* const* d_tab, unsigned nc) {
        msntt::FusedParams F;
        memset(&F, 0, sizeof F);
        F.cols = d_tab;
        F.tw_lo = p->d_tw_lo; F.tw_hi = p->d_tw_hi; F.wr = p->d_wr[0]; F.wr2 = p->d_wr[1];
        F.aux_lo = p->d_aux_lo; F.aux_hi = p->d_aux_hi; F.gtab = p->d_gtab;
        F.log_n = p->log_n; F.lo_bits = p->lo_bits;
        F.nfields = p->nfields[0];
        for (unsigned f = 0; f < F.nfields; f++) F.fields[f] = p->fields[0][f];
        F.scale_const = p->scale_const;
        if (tiny) F.ncols = nc;
        const unsigned pack = tiny ? 16u >> (p->log_n - 8) : 1;   // ntt_fused_tiny, columns per workgroup: 2 / 4 / 8 at 2^11 / 2^10 / 2^9 points
        const dim3 grid((nc + pack - 1) / pack), block(tiny ? msntt::NT : msntt::NT << (p->log_n - 12));
        ProfScope ps(ctx, tiny ? "ntt_fused_tiny" : "ntt_fused_small", 2.0 * col_bytes * nc);
        hipLaunchKernelGGL(k, grid, block, 0, ctx->stream, F);
    });
}

static int lde2_run(ms_ntt_plan* fwd, unsigned log_n, unsigned log_b, const void* const* src, void* const* dst, unsigned ncols, bool natural, unsigned V = 1, ms_ntt_plan* inv = nullptr);

// Inverse transforms of 2^18-point Fp columns through the two forward kernels of the two-pass plan (round 6): the column read backwards is the
// inverse's sum, the forward plan on the subgroup (fwd1) supplies every table, n^-1 h^-k multiplies pass B's natural-order output
// (lde2_kernels.h Params::rev).  Measured, 64 columns: 2.65 -> 2.35 us per column (forward: 2.15).
static int run_inverse_2_18(ms_ntt_plan* p, ms_ntt_plan* fwd1, const void* const* src, void* const* dst, unsigned ncols) {
    ms_ntt_plan* owner = p->base ? p->base : p;                     // the owner's d_oscale: a handle's copy of the plan may predate the table
    MSCHK(plan_oscale(owner));
    return lde2_run(fwd1, 18, 0, src, dst, ncols, true, 1, owner);
}

template <class Params>
static void pass_columns(Params& P, int q, bool last, const void* const* src, void* const* dst, void* scratch, size_t col_bytes, unsigned c0, unsigned nc) {
    for (unsigned c = 0; c < nc; c++) {
        uint64_t* scr = (uint64_t*)((char*)scratch + (size_t)c * col_bytes);
        P.src[c] = (q == 0) ? (const uint64_t*)src[c0 + c] : scr;
        P.dst[c] = last ? (uint64_t*)dst[c0 + c] : scr;
    }
}
// one call of run_passes: what every launch of it shares
struct PassRun {
    ms_ntt_plan* p;
    const void* const* src;
    void* const* dst;
    unsigned valid_rows;
    bool bitrev_out;
    size_t n, col_bytes;
    bool perm;      // uniform-factor plans on Fp columns: pass 1 stores whole lines in a row order that permutes the words inside every run of
                    // 64; pass 2 un-permutes while it reads, in place on the scratch column (its tile owns those 64 words), and the last pass
                    // goes scratch -> dst (natural order, or bit-reversed for the LDE)
    int na;         // sixteenths of pass 1's rows that hold data
};
static bool small_mid_pass(const ms_ntt_plan* p, int q) { return p->uni && q == 1 && p->lr[q] < 8; }
// limb-form radix-256 passes (ntt2_kernels.h) wherever a pass has radix 256 and rows of >= 64 words
// (the per-element scale walk of an inverse coset transform stays with the round-1 last pass: the walk is two table
// loads and a Montgomery product per word, which the 4-wave limb kernel hides worse -- 91 vs 75 us per 2^24
// column; so does the fused bit-reversed store of Fq3 columns, whose runs interleave three words)
static bool limb_pass_ok(const PassRun& R, int q) {
    const ms_ntt_plan* p = R.p;
    const bool last = (q == p->npass - 1);
    const size_t pass_sw = ((size_t)1 << p->log_s[q]) * p->V;
    return small_mid_pass(p, q) || (p->lr[q] == 8 && (R.n * p->V) % msntt2::TILE == 0 &&
           (q == 0 ? ((R.n >> 8) * p->V) % msntt2::TW == 0
                   : (pass_sw % msntt2::TW == 0 && !(last && p->scale_mode == 2 && p->d_scu4 == nullptr) &&
                      !(last && R.bitrev_out && (p->V != 1 || p->inverse || p->scale_mode != 0)))));
}
// Pass q of columns [c0, c0 + nc) on stream st: source -> scratch, scratch in place, scratch -> destination; column c of the range
// goes through scratch column c.  pol: the cache policy of a limb-form pass's tile accesses (ntt2_kernels.h).
static int launch_pass(const PassRun& R, int q, hipStream_t st, unsigned c0, unsigned nc, void* scratch, int pol) {
    ms_ntt_plan* p = R.p;
    ms_ctx* ctx = p->ctx;
    const size_t n = R.n;
    const bool last = (q == p->npass - 1);
    static const char* const pass_names[4] = {"ntt_pass1", "ntt_pass2", "ntt_pass3", "ntt_pass4"};
    ProfScope ps(ctx, pass_names[q], 2.0 * R.col_bytes * nc);
    const bool small_mid = small_mid_pass(p, q);
    const bool v2_ok = limb_pass_ok(R, q);
    if (switches().debug) fprintf(stderr, "[ms_ntt] log_n=%u V=%u pass %d/%d radix 2^%u: %s kernel\n", p->log_n, p->V, q + 1, p->npass, p->lr[q], v2_ok ? (p->uni && q < 2 ? "limb-form (ntt2), uniform inter-pass factor" : "limb-form (ntt2)") : "round-1");
    if (p->uni && q < 2 && !v2_ok) return fail(MS_ERR_INVALID, "internal: uniform inter-pass plan without its limb-form passes");
    if (v2_ok) {
        msntt2::Params Q;
        memset(&Q, 0, sizeof Q);
        pass_columns(Q, q, last, R.src, R.dst, scratch, R.col_bytes, c0, nc);
        Q.wr4 = p->d_wr4[q]; Q.twu4 = p->d_twu4[q]; Q.sc4 = p->d_sc4; Q.scu4 = p->d_scu4; Q.g4 = p->d_g4;
        Q.tw_lo = p->d_tw_lo; Q.tw_hi = p->d_tw_hi; Q.aux_lo = p->d_aux_lo; Q.aux_hi = p->d_aux_hi;
        Q.log_n = p->log_n; Q.V = p->V; Q.valid_rows = R.valid_rows; Q.lo_bits = p->lo_bits; Q.log_s = p->log_s[q];
        Q.tin4 = p->d_tin4; Q.tout4 = p->d_tout4; Q.lq = p->d_lq; Q.r3 = p->lr[2];
        // pass 1 of a uniform-factor plan with last radix 256 (four tiles per block of a row): XCD-aware tile order (ntt2_kernels.h)
        Q.xcd_map = (q == 0 && p->uni && p->V == 1 && p->lr[2] == 8 && (n / msntt2::TILE) % 8 == 0) ? 1u : 0u;
        Q.nfields = p->nfields[q];
        for (unsigned f = 0; f < Q.nfields; f++) Q.fields[f] = p->fields[q][f];
        const K2 k = limb_pass_kernel(pol, p, q, R.na, small_mid, R.perm, R.bitrev_out);
        if (!k) return fail(MS_ERR_INVALID, "internal: no limb-form kernel of pass %d under cache policy %d", q + 1, pol);
        hipLaunchKernelGGL(k, dim3((unsigned)(n * p->V / msntt2::TILE), nc), dim3(msntt2::NT), 0, st, Q);
        return MS_OK;
    }
    msntt::PassParams P;
    memset(&P, 0, sizeof P);
    pass_columns(P, q, last, R.src, R.dst, scratch, R.col_bytes, c0, nc);
    P.tw_lo = p->d_tw_lo; P.tw_hi = p->d_tw_hi; P.wr = p->d_wr[q];
    P.aux_lo = p->d_aux_lo; P.aux_hi = p->d_aux_hi; P.gtab = p->d_gtab;
    P.log_n = p->log_n; P.V = p->V; P.valid_rows = R.valid_rows; P.lo_bits = p->lo_bits; P.log_s = p->log_s[q];
    P.nfields = p->nfields[q];
    for (unsigned f = 0; f < P.nfields; f++) P.fields[f] = p->fields[q][f];
    P.scale_const = p->scale_const;
    const K1 k = q == 0 ? first_pass_r1(p->inverse, !p->inverse && p->coset, R.na) : mid_pass_r1(p->lr[q], p->inverse, last, p->scale_mode, R.bitrev_out);
    if (!k) return fail(MS_ERR_INVALID, "internal: bad pass radix 2^%u", p->lr[q]);
    hipLaunchKernelGGL(k, dim3((unsigned)(n * p->V / msntt::TILE), nc), dim3(msntt::NT), 0, st, P);
    return MS_OK;
}
// side streams 0 .. count-1 start where the context's stream stands / the context's stream goes on when they are done
static int fork_side_streams(ms_ctx* ctx, unsigned count) {
    MSCHK(ctx_side_streams(ctx, count));
    HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
    for (unsigned i = 0; i < count; i++) HIPCHK(hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0));
    return MS_OK;
}
static int join_side_streams(ms_ctx* ctx, unsigned count) {
    for (unsigned i = 0; i < count; i++) {
        HIPCHK(hipEventRecord(ctx->ev_join[i], ctx->side[i]));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
    }
    return MS_OK;
}

// The column chains (profiles/ntt_column_chains.txt).  In batch order a pass covers every column of the group, so pass k + 1 reads a line
// a whole group of traffic after pass k wrote it and every one of the six trips over a column reaches HBM.  Here the columns are dealt
// round-robin to S streams; a stream owns ONE scratch column and runs pass 1 -> 2 -> 3 of its columns one after the other, so the
// intermediate column (written twice, read twice) stays in the 256 MiB Infinity Cache.  Only the side of a pass that touches the column
// itself carries the non-temporal hint.  Ordering is stream order plus the fork and join events: no waiting on the device, the same
// kernels on the same words as the batch.
static bool chains_apply(const PassRun& R, unsigned ncols) {
    const NttSwitches& sw = switches();
    const ms_ntt_plan* p = R.p;
    if (!sw.chains || sw.two_streams || p->ctx->profiling || ncols < 2) return false;      // (profiling: events on one stream, one launch per pass)
    if (!p->uni || p->V != 1 || p->npass != 3 || R.valid_rows != 256 || R.bitrev_out || p->log_n < sw.chain_min_log) return false;
    if (2 * R.col_bytes > ((size_t)256 << 20)) return false;                                // a column and a scratch column fit the cache
    return limb_pass_ok(R, 0) && limb_pass_ok(R, 1) && limb_pass_ok(R, 2);
}
static int run_chains(const PassRun& R, unsigned ncols) {
    ms_ctx* ctx = R.p->ctx;
    const unsigned S = std::min(switches().chain_streams, ncols);
    void* scratch = nullptr;
    MSCHK(ctx_scratch(ctx, (size_t)S * R.col_bytes, &scratch));
    if (switches().debug) fprintf(stderr, "[ms_ntt] log_n=%u: %u columns as chains on %u streams\n", R.p->log_n, ncols, S);
    MSCHK(fork_side_streams(ctx, S - 1));
    static const int policy[3] = {msntt2::POL_NT_LD, msntt2::POL_PLAIN, msntt2::POL_NT_ST};     // pass 2 works on the scratch column alone (hinted stores: slower)
    for (unsigned c = 0; c < ncols; c++) {
        const unsigned s = c % S;
        const hipStream_t st = s == 0 ? ctx->stream : ctx->side[s - 1];
        for (int q = 0; q < 3; q++) MSCHK(launch_pass(R, q, st, c, 1, (char*)scratch + (size_t)s * R.col_bytes, policy[q]));
    }
    MSCHK(join_side_streams(ctx, S - 1));
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// The pass loop: 2 .. 4 passes through a scratch column, each the limb-form kernel (ntt2_kernels.h) where the pass has one, the round-1
// kernel (ntt_kernels.h) otherwise.  valid_rows < 256: pass 1 reads only the first valid_rows/256 of the source; bitrev_out: the last
// pass stores in bit-reversed order.
static int run_passes(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols, unsigned valid_rows, bool bitrev_out) {
    ms_ctx* ctx = p->ctx;
    const NttSwitches& sw = switches();
    PassRun R{p, src, dst, valid_rows, bitrev_out, (size_t)1 << p->log_n, ((size_t)1 << p->log_n) * p->V * 8, p->uni && p->V == 1,
              valid_rows == 64 ? 4 : valid_rows == 32 ? 2 : valid_rows == 16 ? 1 : 16};
    if (chains_apply(R, ncols)) return run_chains(R, ncols);
    const size_t col_bytes = R.col_bytes;
    unsigned group = (unsigned)std::max<size_t>(1, std::min<size_t>(MAXC, ctx->group_bytes / col_bytes));
    group = std::min(group, ncols);
    void* scratch_all = nullptr;
    MSCHK(ctx_scratch(ctx, (size_t)group * col_bytes, &scratch_all));
    // the two-stream split (NttSwitches::two_streams): the halves of a group between a fork and a join event
    const bool two = sw.two_streams && !ctx->profiling && ncols >= 2 && group >= 2 && p->log_n >= sw.two_min_log;
    if (two) MSCHK(fork_side_streams(ctx, 1));
    for (unsigned g0 = 0; g0 < ncols; g0 += group) {
      const unsigned gnc = std::min(group, ncols - g0);
      const unsigned half = (two && gnc >= 2) ? gnc / 2 : gnc;
      for (unsigned s0 = 0; s0 < gnc; s0 = (s0 == 0) ? half : gnc) {     // at most two ranges: [0, half), [half, gnc)
        const unsigned c0 = g0 + s0, nc = (s0 == 0) ? half : gnc - half;
        const hipStream_t st = (s0 == 0) ? ctx->stream : ctx->side[0];
        void* const scratch = (char*)scratch_all + (size_t)s0 * col_bytes;
        for (int q = 0; q < p->npass; q++)
            MSCHK(launch_pass(R, q, st, c0, nc, scratch, beyond_cache(nc, col_bytes) ? msntt2::POL_NT : msntt2::POL_PLAIN));
      }
    }
    if (two) MSCHK(join_side_streams(ctx, 1));
    HIPCHK(hipGetLastError());
    return MS_OK;
}

// Transform `ncols` columns: src[c] -> dst[c] (may alias).  valid_rows < 256 means the
// source only holds the first valid_rows/256 of the domain, the rest is implicit zeros.
int plan_run(ms_ntt_plan* p, const void* const* src, void* const* dst, unsigned ncols, unsigned valid_rows, bool bitrev_out) {
    if (p->is252) {
        if (valid_rows != 256 || bitrev_out) return fail(MS_ERR_INVALID, "internal: Fp252 zero extension / fused bit reversal go through plan_run252_tiled");
        return plan_run252(p, src, dst, ncols);
    }
    if (bitrev_out && p->small) return fail(MS_ERR_INVALID, "internal: fused bit reversal needs the multi-pass path");
    ms_ctx* ctx = p->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const NttSwitches& sw = switches();
    const bool dense = valid_rows == 256 && !bitrev_out;        // the whole column in, natural order out
    const bool fp18 = p->V == 1 && dense && p->log_n == 18;
    // tiny fused: 2^11-point Fp columns; everything else of a small plan (Fq3 columns, MS_NTT_FUSED_SMALL=0) stays with ntt_small
    if (p->small && p->tiny_fused && !sw.fused_off && dense) return run_fused(p, src, dst, ncols);
    if (p->small) {
        if (valid_rows != 256) return fail(MS_ERR_INVALID, "zero-extended input needs a domain of at least 4096 points");
        return run_small(p, src, dst, ncols);
    }
    // Forward transforms of 2^18-point Fp columns: TWO passes -- the coset-LDE kernels with a single coset and natural-order stores
    // (256 x 1024: runs of 16 words in the second pass's stores; from 2^19 on the runs would be 64 bytes and the three-pass plan wins).
    // Measured (profiles/r04_c2_sweep.json): 2.48 -> 2.25 us per column over 64 columns.  At 2^17 the rows are too short for the uniform
    // split of pass A's factor (T = 2) and its per-lane running product loses: 1.50 against 1.37 us -- stays on three passes.
    if (!p->inverse && fp18 && p->d_wr4[0] != nullptr)
        return lde2_run(p->base ? p->base : p, p->log_n, 0, src, dst, ncols, true);   // the CACHED plan owns (and frees) the tables: a handle is a copy
    // ... and the inverse transforms of that size through the same two kernels (run_inverse_2_18)
    if (p->inverse && !sw.inv18_off && fp18) {
        ms_ntt_plan* fwd1 = nullptr;
        MSCHK(ctx_plan(ctx, 1, 18, false, 1, &fwd1));
        if (fwd1->d_wr4[0] != nullptr) return run_inverse_2_18(p, fwd1, src, dst, ncols);
    }
    // fused small: 2^12 .. 2^14-point Fp columns
    if (!sw.fused_off && p->V == 1 && p->log_n >= 12 && p->log_n <= std::min(14u, sw.fused_max) && p->npass == 2 && p->lr[0] == 8 && p->lr[1] == p->log_n - 8 && dense)
        return run_fused(p, src, dst, ncols);
    return run_passes(p, src, dst, ncols, valid_rows, bitrev_out);
}

// ---- two-pass coset LDE (lde2_kernels.h) ------------------------------------------------------------------------------
// fwd = the forward plan of the LDE domain (N = n << log_b points, offset h).  Applies to Fp columns of 2^17..2^22 rows
// (rows of pass B: n / 256 <= 16384 words = one workgroup's tile).
#ifndef MS_LDE2_MAX_LOG_N            // (a build with -DMS_LDE2_MAX_LOG_N=20 is the round-3 dispatch, for before / after timings)
#define MS_LDE2_MAX_LOG_N 22
#endif
// Fq3 columns (V = 3, round 6): 2^18..2^20 rows (rows of pass B: at most 4096 elements -- the three word planes of a row share a workgroup;
// at 2^17 rows the (256, 2, 256) plan is the faster one: 0.37 against 0.49 ms for 9 columns at blow-up 8, profiles/r06_lde_fq3_probe.txt).
static bool lde2_applicable(const ms_ntt_plan* fwd, unsigned V, unsigned log_n, unsigned log_b) {
    const NttSwitches& sw = switches();
    if (V == 3 && (sw.fq3_off || log_n > 20 || (log_n < 18 && !sw.fq3_all))) return false;
    return (V == 1 || V == 3) && log_n >= 17 && log_n <= MS_LDE2_MAX_LOG_N && log_b >= 1 && log_b <= 6 && !fwd->small && fwd->d_wr4[0] != nullptr;
}
// coefficients (2^log_n words per column, src) -> bit-reversed evaluations on the coset of N points (dst, N words per column)
// natural (log_b = 0, 2^17 / 2^18 points): the one coset's transform in natural order -- the forward NTT of the column in two passes
// V = 3: Fq3 columns -- interleaved coefficients in, PLANAR scratch between the passes, interleaved evaluations out (lde2_kernels.h)
static int lde2_run(ms_ntt_plan* fwd, unsigned log_n, unsigned log_b, const void* const* src, void* const* dst, unsigned ncols, bool natural, unsigned V, ms_ntt_plan* inv) {
    ms_ctx* ctx = fwd->ctx;
    hipStream_t st = ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    ms_ntt_plan::Lde2* tb = nullptr;
    MSCHK(lde2_tables(fwd, log_n, log_b, &tb));
    const size_t n = (size_t)1 << log_n, N = n << log_b, col_bytes = N * 8 * V;
    if (V == 3 && natural) return fail(MS_ERR_INVALID, "internal: natural-order two-pass transform is an Fp plan");
    const unsigned T = (unsigned)(n >> 16);
    unsigned group = (unsigned)std::max<size_t>(1, std::min<size_t>(MAXC, ctx->group_bytes / col_bytes));
    group = std::min(group, ncols);
    void* scratch = nullptr;
    MSCHK(ctx_scratch(ctx, (size_t)group * col_bytes, &scratch));
    for (unsigned c0 = 0; c0 < ncols; c0 += group) {
        const unsigned nc = std::min(group, ncols - c0);
        mslde2::Params P;
        memset(&P, 0, sizeof P);
        P.wr4 = fwd->d_wr4[0]; P.gpl = tb->gpl; P.aux = tb->aux; P.t2 = tb->t2; P.tin4 = tb->tin4; P.tout4 = tb->tout4; P.c3 = tb->c3;
        if (inv) {                                              // an inverse transform: the column backwards in, n^-1 h^-k on the way out
            P.rev = 1;
            if (inv->d_oscale) { P.oscale = inv->d_oscale; P.oscale_mode = 2; }
            else { P.oscale_c = inv->scale_const; P.oscale_mode = 1; }
        }
        const bool uni = tb->tin4 != nullptr;
        const bool stream_hint = beyond_cache(nc, col_bytes);
        P.tw_lo = fwd->d_tw_lo; P.tw_hi = fwd->d_tw_hi; P.lo_bits = fwd->lo_bits; P.log_n = log_n; P.log_b = log_b;
        for (unsigned c = 0; c < nc; c++) { P.src[c] = (const uint64_t*)src[c0 + c]; P.dst[c] = (uint64_t*)((char*)scratch + (size_t)c * col_bytes); }
        {
            ProfScope ps(ctx, "lde2_pass_a", (double)(n * 8 * V + col_bytes) * nc);
            if (V != 3 && inv && !uni) return fail(MS_ERR_INVALID, "internal: the backwards pass A is the 2^18-point plan's");
            hipLaunchKernelGGL(lde2_pass_a_kernel(stream_hint, uni, V, inv != nullptr), dim3((unsigned)(n >> 14), V << log_b, nc), dim3(msntt2::NT), 0, st, P);
        }
        for (unsigned c = 0; c < nc; c++) { P.src[c] = (const uint64_t*)((char*)scratch + (size_t)c * col_bytes); P.dst[c] = (uint64_t*)dst[c0 + c]; }
        {
            ProfScope ps(ctx, "lde2_pass_b", 2.0 * col_bytes * nc);
            if (V != 3 && natural && T != 4) return fail(MS_ERR_INVALID, "internal: natural-order two-pass transform is the 2^18-point plan");
            const dim3 g(V == 3 ? 16 * T : 4 * T, nc, 1u << log_b);                     // 64 / T rows per workgroup (Fq3: 16 / T rows x 3 planes)
            const int oscale = inv ? (int)P.oscale_mode : 0;
            const KLde k = stream_hint ? lde2_pass_b_kernel<true>(T, uni, V, natural, oscale) : lde2_pass_b_kernel<false>(T, uni, V, natural, oscale);
            hipLaunchKernelGGL(k, g, dim3(msntt2::NT), 0, st, P);
        }
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}

extern "C" int ms_ntt_encode(ms_ntt_plan* plan, void* d_column) {
    if (!plan || !d_column) return fail(MS_ERR_INVALID, "ms_ntt_encode: null argument");
    if (!user_plan_alive(plan)) return fail(MS_ERR_INVALID, "ms_ntt_encode: the plan's context has been destroyed");
    std::lock_guard<std::mutex> lk(plan->ctx->mu);
    plan->queue.push_back(d_column);
    return MS_OK;
}
// checked mode: the columns of a transform are scanned no later than the launch that would read them -- ms_ntt_encode only queues a pointer,
// ms_ntt_execute checks the queue (as d_column, the name it was handed in under)
static int ntt_enqueue(ms_ntt_plan* plan, void* const* d_columns, unsigned ncols, const char* entry, const char* arg) {
    MSCHK(canon_cols(plan->ctx, entry, arg, field_of_words(plan->V), (size_t)1 << plan->log_n, (const void* const*)d_columns, ncols));
    std::lock_guard<std::mutex> lk(plan->ctx->mu);
    return plan_run(plan, (const void* const*)d_columns, d_columns, ncols, 256);
}
extern "C" int ms_ntt_enqueue(ms_ntt_plan* plan, void* const* d_columns, unsigned ncols) {
    if (!plan || (!d_columns && ncols)) return fail(MS_ERR_INVALID, "ms_ntt_enqueue: null argument");
    if (!user_plan_alive(plan)) return fail(MS_ERR_INVALID, "ms_ntt_enqueue: the plan's context has been destroyed");
    if (ncols == 0) return MS_OK;
    return ntt_enqueue(plan, d_columns, ncols, "ms_ntt_enqueue", "d_columns");
}
extern "C" int ms_ntt_enqueue_to(ms_ntt_plan* plan, const void* const* d_src, void* const* d_dst, unsigned ncols) {
    if (!plan || ((!d_src || !d_dst) && ncols)) return fail(MS_ERR_INVALID, "ms_ntt_enqueue_to: null argument");
    if (!user_plan_alive(plan)) return fail(MS_ERR_INVALID, "ms_ntt_enqueue_to: the plan's context has been destroyed");
    for (unsigned c = 0; c < ncols; c++) if (!d_src[c] || !d_dst[c]) return fail(MS_ERR_INVALID, "ms_ntt_enqueue_to: null column %u", c);
    if (ncols == 0) return MS_OK;
    MSCHK(canon_cols(plan->ctx, "ms_ntt_enqueue_to", "d_src", field_of_words(plan->V), (size_t)1 << plan->log_n, d_src, ncols));
    std::lock_guard<std::mutex> lk(plan->ctx->mu);
    return plan_run(plan, d_src, d_dst, ncols, 256);
}
extern "C" int ms_ntt_execute(ms_ntt_plan* plan) {
    if (!plan) return fail(MS_ERR_INVALID, "ms_ntt_execute: null plan");
    if (!user_plan_alive(plan)) return fail(MS_ERR_INVALID, "ms_ntt_execute: the plan's context has been destroyed");
    std::vector<void*> q;
    { std::lock_guard<std::mutex> lk(plan->ctx->mu); q.swap(plan->queue); }
    if (!q.empty()) MSCHK(ntt_enqueue(plan, q.data(), (unsigned)q.size(), "ms_ntt_execute", "d_column"));
    HIPCHK(hipStreamSynchronize(plan->ctx->stream));
    return MS_OK;
}

// ---------------------------------------------------------------------------------------
// bit reversal
// ---------------------------------------------------------------------------------------
int bit_reverse_run(ms_ctx* ctx, unsigned V, unsigned log_n, const void* const* src, void* const* dst, unsigned ncols) {
    hipStream_t st = ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << log_n;
    if (log_n >= 10 && V != 4) {
        for (unsigned c0 = 0; c0 < ncols; c0 += MAXC) {
            unsigned nc = std::min<unsigned>(MAXC, ncols - c0);
            msntt::BitrevParams B;
            memset(&B, 0, sizeof B);
            for (unsigned c = 0; c < nc; c++) { B.src[c] = (const uint64_t*)src[c0 + c]; B.dst[c] = (uint64_t*)dst[c0 + c]; }
            B.log_n = log_n;
            dim3 grid((unsigned)(n >> 10), nc);
            ProfScope ps(ctx, "bit_reverse", 2.0 * n * V * 8 * nc);
            if (V == 1) hipLaunchKernelGGL(msntt::bit_reverse_tiled<1>, grid, dim3(msntt::NT), 0, st, B);
            else hipLaunchKernelGGL(msntt::bit_reverse_tiled<3>, grid, dim3(msntt::NT), 0, st, B);
        }
    } else {
        // tiny: out of place through scratch when aliased
        const size_t col_bytes = n * V * 8;
        void* scratch = nullptr;
        const unsigned grp = (unsigned)std::max<size_t>(1, std::min<size_t>(MAXC, ((size_t)256 << 20) / col_bytes));
        MSCHK(ctx_scratch(ctx, (size_t)grp * col_bytes, &scratch));
        for (unsigned c0 = 0; c0 < ncols; c0 += grp) {
            unsigned nc = std::min<unsigned>(grp, ncols - c0);
            msntt::BitrevParams B;
            memset(&B, 0, sizeof B);
            for (unsigned c = 0; c < nc; c++) { B.src[c] = (const uint64_t*)src[c0 + c]; B.dst[c] = (uint64_t*)((char*)scratch + c * col_bytes); }
            B.log_n = log_n;
            dim3 grid((unsigned)((n + msntt::NT - 1) / msntt::NT), nc);
            if (V == 1) hipLaunchKernelGGL(msntt::bit_reverse_simple<1>, grid, dim3(msntt::NT), 0, st, B);
            else if (V == 3) hipLaunchKernelGGL(msntt::bit_reverse_simple<3>, grid, dim3(msntt::NT), 0, st, B);
            else hipLaunchKernelGGL(msntt::bit_reverse_simple<4>, grid, dim3(msntt::NT), 0, st, B);
            for (unsigned c = 0; c < nc; c++)
                HIPCHK(hipMemcpyAsync(dst[c0 + c], (char*)scratch + c * col_bytes, col_bytes, hipMemcpyDeviceToDevice, st));
        }
    }
    HIPCHK(hipGetLastError());
    return MS_OK;
}
extern "C" int ms_bit_reverse(ms_ctx* ctx, int field, unsigned log_n, void* const* d_columns, unsigned ncols) {
    if (!ctx || (!d_columns && ncols)) return fail(MS_ERR_INVALID, "ms_bit_reverse: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (log_n > 40) return fail(MS_ERR_INVALID, "log_n too large");
    std::lock_guard<std::mutex> lk(ctx->mu);
    return bit_reverse_run(ctx, V, log_n, (const void* const*)d_columns, d_columns, ncols);
}

// ---------------------------------------------------------------------------------------
// fused LDE, evaluate
// ---------------------------------------------------------------------------------------
// Coefficient columns (2^log_n elements each, src) -> their evaluations on the coset of `fwd`, the forward plan of 2^(log_n + log_b) points,
// in dst; src[c] may be the head of dst[c] (ms_lde).  Goldilocks blow-ups 2^prune_min .. 2^4 take the pruned first pass.  The caller holds ctx->mu.
static int evaluate_on_coset(ms_ctx* ctx, unsigned V, ms_ntt_plan* fwd, unsigned log_n, unsigned log_b, const void* const* src, void* const* dst,
                             unsigned ncols, bool bit_reversed, unsigned prune_min) {
    const unsigned log_N = log_n + log_b;
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N;
    // two-pass coset LDE: beta coset transforms of size n in two passes each, blocks land in the bit-reversed order
    if (V != 4 && lde2_applicable(fwd, V, log_n, log_b)) {
        MSCHK(lde2_run(fwd, log_n, log_b, src, dst, ncols, false, V));
        if (!bit_reversed) MSCHK(bit_reverse_run(ctx, V, log_N, (const void* const*)dst, dst, ncols));
        return MS_OK;
    }
    // 252-bit field, tiled passes: the coefficients are read straight from src (zeros implicit), the bit reversal is part of the last pass
    if (V == 4 && fwd->np252 && log_b <= fwd->lr252[0]) return plan_run252_tiled(fwd, src, dst, ncols, log_b, bit_reversed);
    // pruned first pass: pass 1 reads only the rows that hold coefficients, zero padding is implicit, the bit reversal is fused into the last pass
    if (V != 4 && !fwd->small && log_b >= prune_min && log_b <= 4) return plan_run(fwd, src, dst, ncols, 256u >> log_b, bit_reversed);
    // the plain sequence: copy, explicit zero padding, transform, bit reversal
    for (unsigned c = 0; c < ncols; c++) {
        if (src[c] != dst[c]) HIPCHK(hipMemcpyAsync(dst[c], src[c], n * V * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (N > n) HIPCHK(hipMemsetAsync((char*)dst[c] + n * V * 8, 0, (N - n) * V * 8, ctx->stream));
    }
    MSCHK(plan_run(fwd, (const void* const*)dst, dst, ncols, 256));
    if (bit_reversed) MSCHK(bit_reverse_run(ctx, V, log_N, (const void* const*)dst, dst, ncols));
    return MS_OK;
}

extern "C" int ms_lde(ms_ctx* ctx, int field, unsigned log_n, unsigned log_blowup, const void* h_offset,
                      const void* const* d_in, void* const* d_out, unsigned ncols, int bit_reversed) {
    if (!ctx || !d_in || !d_out) return fail(MS_ERR_INVALID, "ms_lde: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    const unsigned log_N = log_n + log_blowup;
    if (log_N > 40 || (V != 4 && log_N > 32)) return fail(MS_ERR_INVALID, V == 4 ? "LDE domain 2^%u too large" : "LDE domain 2^%u exceeds the two-adicity", log_N);
    MSCHK(canon_host(ctx, "ms_lde", "h_offset", V == 4 ? MS_STARK252_FP : MS_GOLDILOCKS_FP, h_offset, 1));
    MSCHK(canon_cols(ctx, "ms_lde", "d_in", field, (size_t)1 << log_n, d_in, ncols));
    // the inverse transform lands the coefficients in the first 2^log_n elements of the output column
    ms_ntt_plan *inv = nullptr, *fwd = nullptr;
    if (V == 4) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        f252::E h252;
        MSCHK(offset252(h_offset, &h252));
        MSCHK(plan252_cached(ctx, log_n, true, f252::one(), &inv));
        MSCHK(plan252_cached(ctx, log_N, false, h252, &fwd));
        MSCHK(plan_run252(inv, d_in, d_out, ncols));
        return evaluate_on_coset(ctx, V, fwd, log_n, log_blowup, (const void* const*)d_out, d_out, ncols, bit_reversed != 0, 0);
    }
    uint64_t h;
    MSCHK(offset_gl(h_offset, &h));
    std::lock_guard<std::mutex> lk(ctx->mu);
    MSCHK(ctx_plan(ctx, V, log_n, true, 1, &inv));
    MSCHK(ctx_plan(ctx, V, log_N, false, h, &fwd));
    MSCHK(plan_run(inv, d_in, d_out, ncols, 256));
    return evaluate_on_coset(ctx, V, fwd, log_n, log_blowup, (const void* const*)d_out, d_out, ncols, bit_reversed != 0, 0);
}

// Matrix::into_evaluations / bit_reversed_evaluate on columns shorter than the domain (src/matrix.rs:193-251:
// "resize the column to the domain size", i.e. zero-extend the coefficient vector): the second half of ms_lde.
extern "C" int ms_evaluate(ms_ctx* ctx, int field, unsigned log_n, unsigned log_domain, const void* h_offset,
                           const void* const* d_in, void* const* d_out, unsigned ncols, int bit_reversed) {
    if (!ctx || !d_in || !d_out) return fail(MS_ERR_INVALID, "ms_evaluate: null argument");
    unsigned V = 0;
    MSCHK(field_words(field, &V));
    if (log_n > log_domain) return fail(MS_ERR_INVALID, "more coefficients (2^%u) than domain points (2^%u)", log_n, log_domain);
    if (log_domain > 40 || (V != 4 && log_domain > 32)) return fail(MS_ERR_INVALID, V == 4 ? "domain 2^%u too large" : "domain 2^%u exceeds the two-adicity", log_domain);
    MSCHK(canon_host(ctx, "ms_evaluate", "h_offset", V == 4 ? MS_STARK252_FP : MS_GOLDILOCKS_FP, h_offset, 1));
    MSCHK(canon_cols(ctx, "ms_evaluate", "d_in", field, (size_t)1 << log_n, d_in, ncols));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    ms_ntt_plan* fwd = nullptr;
    if (V == 4) {
        f252::E h252;
        MSCHK(offset252(h_offset, &h252));
        MSCHK(plan252_cached(ctx, log_domain, false, h252, &fwd));
    } else {
        uint64_t h;
        MSCHK(offset_gl(h_offset, &h));
        MSCHK(ctx_plan(ctx, V, log_domain, false, h, &fwd));
    }
    // (blow-ups 2^0 and 2^1 copy, pad, transform and bit-reverse separately: the pruned first pass from 2^2 on)
    return evaluate_on_coset(ctx, V, fwd, log_n, log_domain - log_n, d_in, d_out, ncols, bit_reversed != 0, 2);
}

// composition_poly.chunks(k) -> k columns (src/prover.rs:113-121): out[c][j] = in[j*k + c]
extern "C" int ms_deinterleave(ms_ctx* ctx, int field, size_t n_out, unsigned k, const void* d_in, void* const* d_out) {
    if (!ctx || !d_in || !d_out) return fail(MS_ERR_INVALID, "ms_deinterleave: null argument");
    const size_t fb = ms_field_bytes(field);
    if (!fb) return fail(MS_ERR_UNSUPPORTED, "unknown field %d", field);
    if (k == 0 || k > (unsigned)msstage::MAXCOLS) return fail(MS_ERR_UNSUPPORTED, "1..%d columns", msstage::MAXCOLS);
    if (n_out == 0) return MS_OK;
    // element j of column c comes from element j*k + c of d_in, which another lane reads: no column may lie over d_in or over another column
    for (unsigned c = 0; c < k; c++) {
        if (!d_out[c]) return fail(MS_ERR_INVALID, "null column %u", c);
        if (ranges_overlap(d_out[c], n_out * fb, d_in, n_out * k * fb)) return fail(MS_ERR_INVALID, "ms_deinterleave: output column %u and d_in overlap", c);
        for (unsigned f = 0; f < c; f++)
            if (ranges_overlap(d_out[c], n_out * fb, d_out[f], n_out * fb)) return fail(MS_ERR_INVALID, "ms_deinterleave: output columns %u and %u overlap", f, c);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    msscan::DeinterleaveParams P;
    memset(&P, 0, sizeof P);
    for (unsigned c = 0; c < k; c++) P.out[c] = (uint64_t*)d_out[c];
    P.in = (const uint64_t*)d_in; P.n_out = n_out; P.k = k; P.V = (unsigned)(fb / 8);
    const size_t total = n_out * k * P.V;
    ProfScope ps(ctx, "deinterleave", 16.0 * total);
    hipLaunchKernelGGL(msscan::deinterleave, dim3(stream_grid(total)), dim3(msscan::NT), 0, ctx->stream, P);
    HIPCHK(hipGetLastError());
    return MS_OK;
}
