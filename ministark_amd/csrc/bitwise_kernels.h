// Bitwise-operation columns (include/ministark_hip_bitwise.h): a op b on the canonical integers of two columns, the table (op, x, y, x op y)
// over all pairs of `bits`-bit limbs, and that table's multiplicities counted from the word columns.
//   bitwise_columns    grid (blocks, specs), grid-stride, one lane per row: the canonical words of both operands once (Canon<V>::words),
//                      cut to `width` bits, combined word by word, back to Montgomery form, one coalesced store.  The next row's words are
//                      loaded before this row's store goes out.  A lane counts its active and its overflowing rows; a workgroup adds its
//                      sums once (mstab::block_totals).
//   bitwise_col_finish one lane: the report.
//   bitwise_table      grid-stride, one lane per table row: op, x, y, x op y as field elements (all below 2^12: msdc::limb_elem).
//   bitwise_count_plain  grid (blocks, sets), grid-stride, one lane per row: nlimbs adds cnt[slot * 4^bits + (x_j << bits) + y_j] += 1 in
//                      global memory through mslk::count_found, which adds once for the lanes of a wave that hit the wave's first bin.
//                      Correct for every `bits`.
//   bitwise_count_lds  grid (G, nops): workgroup (g, slot) takes its share of the rows of every set whose op has that slot and keeps the
//                      slot's 4^bits bins as a histogram of its own in LDS, then one global add per non-zero bin (msdc::flush_bins).
//                      HB <= 15: 2^HB 32-bit counters, which cannot overflow (the increments of a call are below 2^32).  HB = 16: 2^16 16-bit
//                      counters, two to a word.  A row adds nlimbs increments, all of which may fall on one bin, so the flush interval is
//                      counted in INCREMENTS per lane: at most FLUSH_INCS * LNT <= 65 535 between two flushes, and the low half never
//                      carries into the high one (after a row a workgroup flushes unless another row of the call's most limbs still
//                      fits).  No workgroup waits on another.
//   bitwise_finish     grid-stride: counter -> field element -> d_m, zero past the table; lane 0 writes the report.
// An operand is in range when it is below 2^(nlimbs bits) AS AN INTEGER; a result column is right when every word of it is.
// Integer adds and mins commute: counters and reports are the same on every run.  Every atomic is table_common.h's (plain
// read-modify-write under MS_EMU).  above, limb_elem, the histogram, the writer's parameter record and its report are direct_count.h's,
// which brings lookup_kernels.h (count_found, from_count, Report, EMPTY); Canon and block_totals are table_common.h's.
#pragma once
#include "direct_count.h"

namespace msbw {

static constexpr int NT = msdc::NT, LNT = msdc::LNT, MAXSPECS = 64, MAXSETS = 64, MAXOPS = 3;
static constexpr int OP_AND = 0, OP_OR = 1, OP_XOR = 2;
static constexpr int PACKED_BITS = 8;                     // the limb width whose pair table has 2^16 bins: the packed form
static constexpr int PACKED_MAX_LIMBS = 251 / PACKED_BITS;   // the most limbs a row can have there (Fp252; Fp has 63 / 8)
static constexpr int FLUSH_INCS = msdc::FLUSH_ADDS;       // a row is nlimbs adds: the increments of a lane between two flushes of the packed counters
static_assert(FLUSH_INCS * LNT <= 65535, "a 16-bit counter must not wrap between two flushes: the bound is in increments, not rows");
static_assert(PACKED_MAX_LIMBS <= FLUSH_INCS, "one row's increments must fit between two flushes");

using mstab::mask_holds;
using mstab::add;
using mstab::amin;

__device__ __forceinline__ uint64_t apply(unsigned op, uint64_t x, uint64_t y) { return op == (unsigned)OP_AND ? x & y : op == (unsigned)OP_OR ? x | y : x ^ y; }

// ---- columns ------------------------------------------------------------------------------------------------------------------------
struct Spec {
    const uint64_t* a;
    const uint64_t* b;
    const uint64_t* mask;                     // base column of the activity mask (mask_kind != MASK_ALWAYS)
    uint32_t dst, width, op;
    int32_t mask_kind;
};
using ColParams = msdc::WriterParams<Spec>;

template <int V> struct Pair { uint64_t a[V], b[V]; bool active; };

template <int V>
__device__ __forceinline__ Pair<V> load_pair(const Spec& S, size_t i, size_t n) {
    Pair<V> r;
    #pragma unroll
    for (int l = 0; l < V; l++) { r.a[l] = 0; r.b[l] = 0; }
    r.active = i < n && mask_holds<V>(S.mask, S.mask_kind, i);
    if (r.active) { mstab::Canon<V>::words(S.a, i, r.a); mstab::Canon<V>::words(S.b, i, r.b); }
    return r;
}

// word l of 2^width - 1
__device__ __forceinline__ uint64_t width_mask(unsigned width, int l) {
    const unsigned lo = 64u * l;
    return width <= lo ? 0ull : width >= lo + 64 ? ~0ull : (1ull << (width - lo)) - 1;
}

// an integer below the modulus, least significant word first, in Montgomery form
template <class F> __device__ __forceinline__ typename F::T elem_of(const uint64_t* w);
template <> __device__ __forceinline__ uint64_t elem_of<msstage::FpT>(const uint64_t* w) { return gl::to_mont(w[0]); }
template <> __device__ __forceinline__ f252::E elem_of<msstage::Fp252T>(const uint64_t* w) {
    return (w[0] | w[1] | w[2] | w[3]) ? f252::to_mont(f252::E{{w[0], w[1], w[2], w[3]}}) : f252::zero();
}

// grid (blocks, specs)
template <class F>
__global__ void __launch_bounds__(NT) bitwise_columns(ColParams P) {
    constexpr int V = F::V;
    const Spec S = P.specs[blockIdx.y];
    uint64_t* dst = P.base[S.dst];
    const size_t stride = (size_t)gridDim.x * NT;
    uint64_t nactive = 0, noverflow = 0;
    mstab::FirstRow first{~0ull};
    size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    Pair<V> cur = load_pair<V>(S, i, P.n);
    while (i < P.n) {
        const Pair<V> next = load_pair<V>(S, i + stride, P.n);               // in flight while this row's result goes out
        if (cur.active) {
            nactive++;
            if (msdc::above<V>(cur.a, S.width) || msdc::above<V>(cur.b, S.width)) { noverflow++; first.see(blockIdx.y, i); }
        }
        uint64_t r[V];                                                         // an inactive row's words are zero, and so is 0 op 0
        #pragma unroll
        for (int l = 0; l < V; l++) { const uint64_t wm = width_mask(S.width, l); r[l] = apply(S.op, cur.a[l] & wm, cur.b[l] & wm); }
        F::store(dst, i, elem_of<F>(r));
        cur = next;
        i += stride;
    }
    mstab::block_totals(nactive, noverflow, first.at, P.active, P.overflow, P.first);
}

static __global__ void bitwise_col_finish(ColParams P) { msdc::write_limb_report(P); }

// ---- the table ----------------------------------------------------------------------------------------------------------------------
struct TableParams {
    uint64_t* top;                            // null: no op column
    uint64_t* tx;
    uint64_t* ty;
    uint64_t* tz;
    size_t n_t, T;
    unsigned bits, ops[MAXOPS];
};

template <class F>
__global__ void __launch_bounds__(NT) bitwise_table(TableParams P) {
    const uint32_t lmask = (1u << P.bits) - 1;
    for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < P.n_t; j += (size_t)gridDim.x * NT) {
        const uint32_t r = (uint32_t)(j < P.T ? j : P.T - 1);
        const unsigned s = r >> (2 * P.bits);
        const unsigned op = s == 0 ? P.ops[0] : s == 1 ? P.ops[1] : P.ops[2];
        const uint32_t x = (r >> P.bits) & lmask, y = r & lmask;
        if (P.top) F::store(P.top, j, msdc::limb_elem<F>(op));
        F::store(P.tx, j, msdc::limb_elem<F>(x));
        F::store(P.ty, j, msdc::limb_elem<F>(y));
        F::store(P.tz, j, msdc::limb_elem<F>((uint32_t)apply(op, x, y)));
    }
}

// ---- counts -------------------------------------------------------------------------------------------------------------------------
struct Set {
    const uint64_t* a;
    const uint64_t* b;
    const uint64_t* c;                        // null: no result column to check
    const uint64_t* mask;
    int32_t mask_kind;
    uint32_t op, slot, nlimbs;
};
struct CountParams {
    Set sets[MAXSETS];
    uint32_t* cnt;                            // [T], zero before the count
    uint64_t* first;                          // min over the missing rows of (set << 32 | row); all ones
    uint64_t* missing;                        // zero
    uint64_t* m;
    mslk::Report* report;
    size_t n, n_m, T;
    unsigned bits, nsets, max_limbs;          // max_limbs: the most limbs a set of the call has
};

// the operands of an active row -> are they below 2^(nlimbs bits), and is the result column, if there is one, a op b?
template <int V>
__device__ __forceinline__ bool load_operands(const Set& L, size_t i, unsigned bits, uint64_t* wa, uint64_t* wb) {
    mstab::Canon<V>::words(L.a, i, wa);
    mstab::Canon<V>::words(L.b, i, wb);
    const unsigned total = L.nlimbs * bits;
    bool ok = !msdc::above<V>(wa, total) && !msdc::above<V>(wb, total);
    if (L.c) {
        uint64_t wc[V], diff = 0;
        mstab::Canon<V>::words(L.c, i, wc);
        #pragma unroll
        for (int l = 0; l < V; l++) diff |= wc[l] ^ apply(L.op, wa[l], wb[l]);
        ok = ok && diff == 0;
    }
    return ok;
}

// the low `bits` bits of the 64 V-bit integer w, which is shifted right by as many: 1 <= bits <= 12.  The limbs of a row come out one
// after another, a limb that straddles two words included, and every index is a constant: range_kernels.h's limb_at picks the word a limb starts in,
// which here, with two operands in flight, made the compiler keep both in LDS (and in scratch where the histogram left no room).
template <int V>
__device__ __forceinline__ uint32_t pop_limb(uint64_t* w, unsigned bits) {
    const uint32_t x = (uint32_t)w[0] & ((1u << bits) - 1);
    #pragma unroll
    for (int l = 0; l + 1 < V; l++) w[l] = w[l] >> bits | w[l + 1] << (64 - bits);
    w[V - 1] >>= bits;
    return x;
}

// grid (blocks, sets)
template <int V>
__global__ void __launch_bounds__(NT) bitwise_count_plain(CountParams P) {
    const Set& L = P.sets[blockIdx.y];
    const unsigned bits = P.bits, nlimbs = L.nlimbs;
    uint32_t* cnt = P.cnt + ((size_t)L.slot << (2 * bits));
    uint64_t missing = 0;
    mstab::FirstRow first{~0ull};
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += (size_t)gridDim.x * NT) {
        uint64_t wa[V], wb[V];
        #pragma unroll
        for (int l = 0; l < V; l++) { wa[l] = 0; wb[l] = 0; }
        bool counted = false;
        if (mask_holds<V>(L.mask, L.mask_kind, i)) {
            counted = load_operands<V>(L, i, bits, wa, wb);
            if (!counted) { missing++; first.see(blockIdx.y, i); }
        }
        for (unsigned j = 0; j < nlimbs; j++) {                                // the same trip count on every lane that is here
            const uint32_t x = pop_limb<V>(wa, bits), y = pop_limb<V>(wb, bits);
            mslk::count_found<true>(cnt, counted ? (x << bits | y) : mslk::EMPTY);
        }
    }
    if (missing) { add(P.missing, missing); amin(P.first, first.at); }
}

// grid (G, nops): workgroup (g, slot) takes rows g * LNT + lane, + G * LNT, ... of every set of that slot.  2 bits <= HB.
template <int V, int HB>
__global__ void __launch_bounds__(LNT) bitwise_count_lds(CountParams P) {
    __shared__ uint32_t hist[msdc::hist_words<HB>];
    const unsigned bits = P.bits, slot = blockIdx.y;
    const unsigned nwords = HB <= 15 ? 1u << (2 * bits) : 1u << 15;
    uint32_t* cnt = P.cnt + ((size_t)slot << (2 * bits));
    msdc::hist_clear(hist, nwords);
    uint64_t missing = 0;
    mstab::FirstRow first{~0ull};
    unsigned pending = 0;                                                      // increments a lane may have made since the last flush
    for (unsigned s = 0; s < P.nsets; s++) {
        const Set& L = P.sets[s];
        if (L.slot != slot) continue;
        const unsigned nlimbs = L.nlimbs;
        // the trip count is the workgroup's, not the lane's: every lane reaches the flush's barriers
        for (size_t row0 = (size_t)blockIdx.x * LNT; row0 < P.n; row0 += (size_t)gridDim.x * LNT) {
            const size_t i = row0 + threadIdx.x;
            if (i < P.n && mask_holds<V>(L.mask, L.mask_kind, i)) {
                uint64_t wa[V], wb[V];
                if (!load_operands<V>(L, i, bits, wa, wb)) { missing++; first.see(s, i); }
                else {
                    for (unsigned j = 0; j < nlimbs; j++) {
                        const uint32_t x = pop_limb<V>(wa, bits), y = pop_limb<V>(wb, bits);
                        msdc::hist_add<HB>(hist, x << bits | y);
                    }
                }
            }
            // the flush FOLLOWS the row's adds, as in range_count_lds: with the check in front of them the compiler left out the wait for
            // the LDS adds before the flush's first barrier, and an add that landed between a lane's read of a word and its clearing of it
            // was lost (a few counts in 10^8 on a hot bin; tests/test_bitwise_abi.py reads the assembly for that wait).  Whatever the next
            // row's set is, it adds at most max_limbs.
            if (HB > 15) {
                pending += nlimbs;
                if (pending + P.max_limbs > (unsigned)FLUSH_INCS) { msdc::flush_bins<HB>(hist, cnt, nwords); pending = 0; }
            }
        }
    }
    msdc::flush_bins<HB>(hist, cnt, nwords);
    if (missing) { add(P.missing, missing); amin(P.first, first.at); }
}

template <class F>
__global__ void __launch_bounds__(NT) bitwise_finish(CountParams P) {
    for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < P.n_m; j += (size_t)gridDim.x * NT)
        F::store(P.m, j, mslk::from_count<F>(j < P.T ? P.cnt[j] : 0u));
    if (blockIdx.x == 0 && threadIdx.x == 0) mslk::write_report(P.report, *P.missing, *P.first, 0);
}

}  // namespace msbw
