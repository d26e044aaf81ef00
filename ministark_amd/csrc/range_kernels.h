// Range-check columns (include/ministark_hip_range.h): the limbs of a value column, and the multiplicities of the table 0 .. 2^bits - 1.
//   limb_decompose  grid (blocks, specs), grid-stride, one lane per row: the canonical words of the value once (Canon<V>::words), limb j =
//                   bits [j * bits, (j + 1) * bits) of them -- a limb may straddle two 64-bit words -- back to Montgomery form, one coalesced
//                   store per limb column.  The next row's words are loaded before this row's stores go out.  A lane counts its active
//                   and its overflowing rows; a workgroup adds its sums once (mstab::block_totals: through the wave, then LDS).
//   limb_finish     one lane: the report.
//   range_count_plain  grid (blocks, sets), grid-stride, one lane per row: cnt[v] += 1 in global memory through mslk::count_found, which
//                   adds once for the lanes of a wave that hit the wave's first bin.  Correct for every `bits`.
//   range_count_lds    G workgroups of LNT lanes, each over its share of the rows of EVERY set: a histogram of its own in LDS, then one
//                   global add per non-zero bin.  HB <= 15: 2^HB 32-bit counters, which cannot overflow (sets * rows < 2^32).  HB = 16:
//                   2^16 16-bit counters, two to a word, flushed after at most FLUSH_ROUNDS * LNT <= 65 535 counted rows, so that the
//                   low half never carries into the high one.  No workgroup waits on another.  The histogram itself is direct_count.h's.
//   range_finish    grid-stride: counter -> field element -> d_m, zero past the table; lane 0 writes the report.
// A value is in the table when it is below 2^bits AS AN INTEGER: every word above the first has to be zero.
// Integer adds and mins commute: counters and reports are the same on every run.  Every atomic is table_common.h's (plain
// read-modify-write under MS_EMU, where the lanes of a launch run one after another).  above, limb_elem, the histogram, the writer's
// parameter record and its report are direct_count.h's, which brings lookup_kernels.h (count_found, from_count, Report, EMPTY).
#pragma once
#include "direct_count.h"

namespace msrg {

static constexpr int NT = msdc::NT, LNT = msdc::LNT, MAXSPECS = 64, MAXSETS = 64;
static constexpr int FLUSH_ROUNDS = msdc::FLUSH_ADDS;     // a row is one add: the rounds of a workgroup between two flushes of the packed counters
static_assert(FLUSH_ROUNDS * LNT <= 65535, "a 16-bit counter must not wrap between two flushes");

using mstab::mask_holds;
using mstab::add;
using mstab::amin;

// ---- limbs --------------------------------------------------------------------------------------------------------------------------
struct Spec {
    const uint64_t* src;
    const uint64_t* mask;                     // base column of the activity mask (mask_kind != MASK_ALWAYS)
    uint32_t dst0, nlimbs, bits;
    int32_t mask_kind;
};
using LimbParams = msdc::WriterParams<Spec>;

template <int V> struct Row { uint64_t w[V]; bool active; };

template <int V>
__device__ __forceinline__ Row<V> load_row(const Spec& S, size_t i, size_t n) {
    Row<V> r;
    #pragma unroll
    for (int l = 0; l < V; l++) r.w[l] = 0;
    r.active = i < n && mask_holds<V>(S.mask, S.mask_kind, i);
    if (r.active) mstab::Canon<V>::words(S.src, i, r.w);
    return r;
}

// word k < V of w, by selects: an index the compiler cannot see through would put w into scratch memory
template <int V>
__device__ __forceinline__ uint64_t word_at(const uint64_t* w, unsigned k) {
    uint64_t r = w[0];
    #pragma unroll
    for (int l = 1; l < V; l++) if (k == (unsigned)l) r = w[l];
    return r;
}

// bits [pos, pos + bits) of the 64 V-bit integer w, 1 <= bits <= 32, pos + bits <= 64 V
template <int V>
__device__ __forceinline__ uint32_t limb_at(const uint64_t* w, unsigned pos, unsigned bits) {
    const unsigned k = pos >> 6, sh = pos & 63u;
    uint64_t x = word_at<V>(w, k) >> sh;
    if (sh + bits > 64) x |= word_at<V>(w, k + 1 < (unsigned)V ? k + 1 : (unsigned)V - 1) << (64 - sh);      // sh > 32 here: the shift is 1 .. 31
    return (uint32_t)(x & ((1ull << bits) - 1));
}

// grid (blocks, specs)
template <class F>
__global__ void __launch_bounds__(NT) limb_decompose(LimbParams P) {
    constexpr int V = F::V;
    const Spec S = P.specs[blockIdx.y];
    uint64_t* const* dst = P.base + S.dst0;
    const size_t stride = (size_t)gridDim.x * NT;
    uint64_t nactive = 0, noverflow = 0;
    mstab::FirstRow first{~0ull};
    size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    Row<V> cur = load_row<V>(S, i, P.n);
    while (i < P.n) {
        const Row<V> next = load_row<V>(S, i + stride, P.n);                 // in flight while this row's limbs go out
        if (cur.active) {
            nactive++;
            if (msdc::above<V>(cur.w, S.nlimbs * S.bits)) { noverflow++; first.see(blockIdx.y, i); }
        }
        for (unsigned j = 0; j < S.nlimbs; j++)                                // an inactive row's words are zero, and so are its limbs
            F::store(dst[j], i, msdc::limb_elem<F>(limb_at<V>(cur.w, j * S.bits, S.bits)));
        cur = next;
        i += stride;
    }
    mstab::block_totals(nactive, noverflow, first.at, P.active, P.overflow, P.first);
}

static __global__ void limb_finish(LimbParams P) { msdc::write_limb_report(P); }

// ---- counts -------------------------------------------------------------------------------------------------------------------------
struct Set {
    const uint64_t* col;
    const uint64_t* mask;
    int32_t mask_kind, pad;
};
struct CountParams {
    Set sets[MAXSETS];
    uint32_t* cnt;                            // [2^bits], zero before the count
    uint64_t* first;                          // min over the missing rows of (set << 32 | row); all ones
    uint64_t* missing;                        // zero
    uint64_t* m;
    mslk::Report* report;
    size_t n, n_m;
    unsigned bits, nsets;
};

// the bin of an active row, or mslk::EMPTY for a value that is not below 2^bits (bits <= 24: no bin is EMPTY)
template <int V>
__device__ __forceinline__ uint32_t bin_of(const uint64_t* col, size_t i, unsigned bits) {
    uint64_t w[V];
    mstab::Canon<V>::words(col, i, w);
    uint64_t high = w[0] >> bits;
    #pragma unroll
    for (int l = 1; l < V; l++) high |= w[l];
    return high ? mslk::EMPTY : (uint32_t)w[0];
}

// grid (blocks, sets)
template <int V>
__global__ void __launch_bounds__(NT) range_count_plain(CountParams P) {
    const Set& L = P.sets[blockIdx.y];
    uint64_t missing = 0;
    mstab::FirstRow first{~0ull};
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += (size_t)gridDim.x * NT) {
        uint32_t found = mslk::EMPTY;
        if (mask_holds<V>(L.mask, L.mask_kind, i)) {
            found = bin_of<V>(L.col, i, P.bits);
            if (found == mslk::EMPTY) { missing++; first.see(blockIdx.y, i); }
        }
        mslk::count_found<true>(P.cnt, found);
    }
    if (missing) { add(P.missing, missing); amin(P.first, first.at); }
}

// grid (G): workgroup b takes rows b * LNT + lane, + G * LNT, ... of every set.  bits <= HB.
template <int V, int HB>
__global__ void __launch_bounds__(LNT) range_count_lds(CountParams P) {
    __shared__ uint32_t hist[msdc::hist_words<HB>];
    const unsigned nwords = HB <= 15 ? 1u << P.bits : 1u << 15;
    msdc::hist_clear(hist, nwords);
    uint64_t missing = 0;
    mstab::FirstRow first{~0ull};
    int rounds = 0;
    for (unsigned s = 0; s < P.nsets; s++) {
        const Set& L = P.sets[s];
        // the trip count is the workgroup's, not the lane's: every lane reaches the flush's barriers
        for (size_t row0 = (size_t)blockIdx.x * LNT; row0 < P.n; row0 += (size_t)gridDim.x * LNT) {
            const size_t i = row0 + threadIdx.x;
            if (i < P.n && mask_holds<V>(L.mask, L.mask_kind, i)) {
                const uint32_t v = bin_of<V>(L.col, i, P.bits);
                if (v == mslk::EMPTY) { missing++; first.see(s, i); }
                else msdc::hist_add<HB>(hist, v);
            }
            if (HB > 15 && ++rounds == FLUSH_ROUNDS) { msdc::flush_bins<HB>(hist, P.cnt, nwords); rounds = 0; }
        }
    }
    msdc::flush_bins<HB>(hist, P.cnt, nwords);
    if (missing) { add(P.missing, missing); amin(P.first, first.at); }
}

template <class F>
__global__ void __launch_bounds__(NT) range_finish(CountParams P) {
    const size_t bins = (size_t)1 << P.bits;
    for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < P.n_m; j += (size_t)gridDim.x * NT)
        F::store(P.m, j, mslk::from_count<F>(j < bins ? P.cnt[j] : 0u));
    if (blockIdx.x == 0 && threadIdx.x == 0) mslk::write_report(P.report, *P.missing, *P.first, 0);
}

}  // namespace msrg
