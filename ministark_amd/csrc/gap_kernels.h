// Deriving a padded table where the trace lies: select rows, fill clock gaps, pad (include/ministark_hip_gaps.h).
//     cnt(j) = act(j) ? 1 + gap(j) : 0      start = the exclusive prefix of cnt      output row j comes from position s, start[s] <= j
// The plan is three launches and the fill one.  No workgroup waits on another: whatever a launch needs from all workgroups of an earlier
// one is a launch boundary away.  No look-back, and no rank or position is taken from an atomic: the atomics only add, max and min integers
// into the report, which commute, so the result is the same on every run.
//   gap_count    per tile of TILE positions: the mask, the canonical counter out of Montgomery form into LDS (TILE + 1 of them: the first
//                position of the next tile is the last one's neighbour, so a pair that straddles a tile or a wave edge is like any other),
//                gap(j) from the integer difference to the neighbour, cnt(j) into start[j]; the tile's sum into tile_sum[tile]; the
//                report's sums, max and min reduced registers -> wave -> LDS -> one integer atomic per workgroup and quantity.
//   gap_scan     one workgroup: the exclusive prefix of tile_sum[] in place, in rounds of SCAN_ROUND tiles with a carry; start[n] and
//                report.rows_out.
//   gap_starts   per tile: start[j] = tile offset + the exclusive prefix of cnt inside the tile (a thread takes ITEMS consecutive positions).
//   gap_fill     output-centric: a workgroup owns OUT_TILE output rows of one column (columns on grid.y), so one row with a gap of a million
//                costs what a million rows cost.  Two searches find the slice of start[] that covers the tile; a slice of at most SLICE
//                entries is staged in LDS and every thread searches there, a longer one (runs of inactive positions) is searched in global
//                memory.  k = j - start[s] goes into Montgomery form with the field's own product.
#pragma once
#include "table_common.h"

namespace msgap {

static constexpr int NT = 256, ITEMS = 4, TILE = NT * ITEMS, SCAN_ROUND = NT, OUT_ITEMS = 4, OUT_TILE = NT * OUT_ITEMS, SLICE = 2048;
static constexpr int MAXGROUP = 3, MAXCOLS = 128;
static constexpr int COPY = 0, ZERO = 1, COUNTER = 2, FLAG = 3;
static constexpr uint64_t GAP_CAP = 1ull << 32;

using mstab::mask_holds;
using mstab::Canon;
using mstab::add;
using mstab::amax;
using mstab::amin;
using mstab::block_exclusive;

struct Report { uint64_t active, rows_out, gaps, max_gap, unordered, first_unordered, saturated, pad0; };
// the quantities a workgroup reduces, in the order of its LDS slots
enum { Q_SUM = 0, Q_ACTIVE, Q_GAPS, Q_UNORDERED, Q_SATURATED, Q_MAX, Q_FIRST, NQ };

struct PlanParams {
    const uint64_t* group[MAXGROUP];          // group[0 .. ngroup), Montgomery form
    const uint64_t* counter;                  // or null: no gaps
    const uint64_t* mask;                     // mask_kind != MASK_ALWAYS
    const uint32_t* perm;                     // or null: the identity
    uint64_t* start;                          // [n + 1]
    uint64_t* tile_sum;                       // [ntiles]
    Report* report;
    uint64_t n_src;
    uint32_t n, ntiles, ngroup;
    int32_t mask_kind;
};

// b - a over V words: -> 0 when b <= a (unordered), else gap = min(b - a - 1, 2^32) and *clipped when b - a - 1 > 2^32
template <int V>
__device__ __forceinline__ bool difference(const uint64_t* a, const uint64_t* b, uint64_t* gap, bool* clipped) {
    uint64_t d[V];
    uint64_t borrow = 0, any = 0;
    #pragma unroll
    for (int l = 0; l < V; l++) {
        const uint64_t x = b[l] - a[l], y = x - borrow;
        borrow = (uint64_t)(b[l] < a[l]) | (uint64_t)(x < borrow);
        d[l] = y;
        any |= y;
    }
    if (borrow || any == 0) return false;
    uint64_t high = 0;
    #pragma unroll
    for (int l = 1; l < V; l++) high |= d[l];
    const uint64_t g = d[0] - 1;                                               // with a high word set, d - 1 >= 2^64 - 1 whatever d[0] is
    *clipped = high != 0 || g > GAP_CAP;
    *gap = *clipped ? GAP_CAP : g;
    return true;
}

template <int V>
__global__ void __launch_bounds__(NT) gap_count(PlanParams P) {
    __shared__ uint64_t s_canon[(TILE + 1) * V];
    __shared__ uint8_t s_act[TILE + 1];
    __shared__ uint64_t s_q[NQ];
    if (threadIdx.x < NQ) s_q[threadIdx.x] = threadIdx.x == Q_FIRST ? ~0ull : 0ull;
    const size_t n = P.n, first = (size_t)blockIdx.x * TILE;
    // the tile's positions and the first of the next: is it active, and the canonical counter
    for (uint32_t t = threadIdx.x; t <= (uint32_t)TILE; t += NT) {
        const size_t j = first + t;
        bool act = false;
        if (j < n) {
            const size_t row = P.perm ? (size_t)P.perm[j] : j;
            if (row < P.n_src) {
                act = mask_holds<V>(P.mask, P.mask_kind, row);
                if (act && P.counter) Canon<V>::words(P.counter, row, s_canon + (size_t)t * V);
            }
        }
        s_act[t] = act;
    }
    __syncthreads();
    uint64_t sum = 0, nact = 0, ngaps = 0, nun = 0, nsat = 0, vmax = 0, vfirst = ~0ull;
    #pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t t = i * NT + threadIdx.x;
        const size_t j = first + t;
        if (j < n) {
            uint64_t cnt = 0;
            if (s_act[t]) {
                uint64_t gap = 0;
                if (P.counter && s_act[t + 1]) {                                  // s_act[t + 1] is false past the last position
                    const size_t r0 = P.perm ? (size_t)P.perm[j] : j, r1 = P.perm ? (size_t)P.perm[j + 1] : j + 1;
                    uint64_t differ = 0;
                    #pragma unroll
                    for (int g = 0; g < MAXGROUP; g++) {
                        if ((uint32_t)g < P.ngroup) {
                            #pragma unroll
                            for (int l = 0; l < V; l++) differ |= P.group[g][r0 * V + l] ^ P.group[g][r1 * V + l];
                        }
                    }
                    if (!differ) {
                        bool clipped = false;
                        if (difference<V>(s_canon + (size_t)t * V, s_canon + (size_t)(t + 1) * V, &gap, &clipped)) nsat += clipped;
                        else { nun++; vfirst = vfirst < (uint64_t)j ? vfirst : (uint64_t)j; }
                    }
                }
                cnt = 1 + gap;
                nact++;
                ngaps += gap != 0;
                vmax = vmax > gap ? vmax : gap;
            }
            P.start[j] = cnt;
            sum += cnt;
        }
    }
#ifndef MS_EMU
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += (uint64_t)__shfl_xor((unsigned long long)sum, d);
        nact += (uint64_t)__shfl_xor((unsigned long long)nact, d);
        ngaps += (uint64_t)__shfl_xor((unsigned long long)ngaps, d);
        nun += (uint64_t)__shfl_xor((unsigned long long)nun, d);
        nsat += (uint64_t)__shfl_xor((unsigned long long)nsat, d);
        const uint64_t om = (uint64_t)__shfl_xor((unsigned long long)vmax, d), of = (uint64_t)__shfl_xor((unsigned long long)vfirst, d);
        vmax = vmax > om ? vmax : om;
        vfirst = vfirst < of ? vfirst : of;
    }
    const bool speaker = (threadIdx.x & 63u) == 0;
#else
    const bool speaker = true;
#endif
    if (speaker) {
        add(&s_q[Q_SUM], sum); add(&s_q[Q_ACTIVE], nact); add(&s_q[Q_GAPS], ngaps); add(&s_q[Q_UNORDERED], nun); add(&s_q[Q_SATURATED], nsat);
        amax(&s_q[Q_MAX], vmax); amin(&s_q[Q_FIRST], vfirst);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        P.tile_sum[blockIdx.x] = s_q[Q_SUM];
        if (s_q[Q_ACTIVE]) add(&P.report->active, s_q[Q_ACTIVE]);
        if (s_q[Q_GAPS]) add(&P.report->gaps, s_q[Q_GAPS]);
        if (s_q[Q_UNORDERED]) add(&P.report->unordered, s_q[Q_UNORDERED]);
        if (s_q[Q_SATURATED]) add(&P.report->saturated, s_q[Q_SATURATED]);
        if (s_q[Q_MAX]) amax(&P.report->max_gap, s_q[Q_MAX]);
        if (s_q[Q_FIRST] != ~0ull) amin(&P.report->first_unordered, s_q[Q_FIRST]);
    }
}

__global__ void __launch_bounds__(NT) gap_scan(PlanParams P) {
    __shared__ uint64_t s_a[NT], s_b[NT];
    const uint64_t carry = mstab::prefix_in_rounds(P.tile_sum, P.ntiles, (unsigned)SCAN_ROUND, s_a, s_b);
    if (threadIdx.x == 0) { P.start[P.n] = carry; P.report->rows_out = carry; }
}

__global__ void __launch_bounds__(NT) gap_starts(PlanParams P) {
    __shared__ uint64_t s_a[NT], s_b[NT];
    const size_t n = P.n, first = (size_t)blockIdx.x * TILE + (size_t)threadIdx.x * ITEMS;
    uint64_t c[ITEMS], mine = 0;
    #pragma unroll
    for (int i = 0; i < ITEMS; i++) { c[i] = first + i < n ? P.start[first + i] : 0ull; mine += c[i]; }
    uint64_t sum;
    uint64_t at = P.tile_sum[blockIdx.x] + block_exclusive(mine, (unsigned)NT, s_a, s_b, &sum);
    #pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        if (first + i < n) P.start[first + i] = at;
        at += c[i];
    }
}

struct FillParams {
    const uint64_t* src[MAXCOLS];             // null for FLAG
    uint64_t* dst[MAXCOLS];
    uint8_t kind[MAXCOLS];
    const uint32_t* perm;                     // or null
    const uint64_t* start;                    // [n + 1]
    uint64_t n_src, n_out;
    uint32_t n, pad;
};

// the number of entries of a[0 .. len) that are <= v, for ascending a; any a: a value in [0, len]
__device__ __forceinline__ uint32_t count_le(const uint64_t* a, uint32_t len, uint64_t v) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <int V> struct Elem;
template <> struct Elem<1> {
    static __device__ __forceinline__ void plus(uint64_t* e, uint64_t k) { e[0] = gl::add(gl::canon(e[0]), gl::to_mont(gl::canon(k))); }
    static __device__ __forceinline__ void one(uint64_t* e) { e[0] = gl::ONE_MONT; }
};
template <> struct Elem<4> {
    static __device__ __forceinline__ void plus(uint64_t* e, uint64_t k) {
        const f252::E s = f252::add(f252::E{{e[0], e[1], e[2], e[3]}}, f252::to_mont(f252::E{{k, 0, 0, 0}}));
        e[0] = s.l[0]; e[1] = s.l[1]; e[2] = s.l[2]; e[3] = s.l[3];
    }
    static __device__ __forceinline__ void one(uint64_t* e) { const f252::E o = f252::one(); e[0] = o.l[0]; e[1] = o.l[1]; e[2] = o.l[2]; e[3] = o.l[3]; }
};

// grid (output tiles, columns)
template <int V>
__global__ void __launch_bounds__(NT) gap_fill(FillParams P) {
    __shared__ uint64_t s_slice[SLICE];
    __shared__ uint32_t s_edge[2];
    const uint64_t* src = P.src[blockIdx.y];
    uint64_t* dst = P.dst[blockIdx.y];
    const int kind = P.kind[blockIdx.y];
    const uint64_t rows_out = P.n ? P.start[P.n] : 0ull;
    const uint64_t o0 = (uint64_t)blockIdx.x * OUT_TILE;
    const uint64_t o1 = o0 + OUT_TILE < P.n_out ? o0 + OUT_TILE : P.n_out;     // the tile's output rows [o0, o1), o0 < o1
    if (rows_out == 0) {
        #pragma unroll
        for (int i = 0; i < OUT_ITEMS; i++) {
            const uint64_t j = o0 + (uint64_t)i * NT + threadIdx.x;
            if (j < o1) {
                uint64_t e[V];
                #pragma unroll
                for (int l = 0; l < V; l++) e[l] = 0;
                if (kind == FLAG) Elem<V>::one(e);
                #pragma unroll
                for (int l = 0; l < V; l++) dst[j * V + l] = e[l];
            }
        }
        return;
    }
    // the positions of the tile's first and last row: s = (the entries of start[0 .. n) that are <= jj) - 1, at least 0
    if (threadIdx.x < 2) {
        const uint64_t j = threadIdx.x == 0 ? o0 : o1 - 1, jj = j < rows_out - 1 ? j : rows_out - 1;
        const uint32_t c = count_le(P.start, P.n, jj);
        s_edge[threadIdx.x] = c ? c - 1 : 0u;
    }
    __syncthreads();
    const uint32_t s_lo = s_edge[0], s_hi = s_edge[1] > s_edge[0] ? s_edge[1] : s_edge[0];            // in [0, n), s_lo <= s_hi
    const uint32_t len = s_hi - s_lo + 1;
    const bool staged = len <= (uint32_t)SLICE;
    if (staged) {
        for (uint32_t t = threadIdx.x; t < len; t += NT) s_slice[t] = P.start[s_lo + t];
        __syncthreads();
    }
    const uint64_t* slice = staged ? s_slice : P.start + s_lo;
    #pragma unroll
    for (int i = 0; i < OUT_ITEMS; i++) {
        const uint64_t j = o0 + (uint64_t)i * NT + threadIdx.x;
        if (j < o1) {
            const uint64_t jj = j < rows_out - 1 ? j : rows_out - 1;
            const uint32_t c = count_le(slice, len, jj);
            const uint32_t at = c ? c - 1 : 0u;
            const uint32_t s = s_lo + at;
            const uint64_t k = j - slice[at];
            uint64_t e[V];
            #pragma unroll
            for (int l = 0; l < V; l++) e[l] = 0;
            if (kind == FLAG) {
                if (k != 0) Elem<V>::one(e);
            } else if (kind != ZERO || k == 0) {
                const size_t row = P.perm ? (size_t)P.perm[s] : (size_t)s;
                if (row < P.n_src) {
                    #pragma unroll
                    for (int l = 0; l < V; l++) e[l] = src[row * V + l];
                }
                if (kind == COUNTER && k != 0) Elem<V>::plus(e, k);
            }
            #pragma unroll
            for (int l = 0; l < V; l++) dst[j * V + l] = e[l];
        }
    }
}

}  // namespace msgap
