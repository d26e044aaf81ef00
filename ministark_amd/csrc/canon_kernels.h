// Canonical-form scan (ms_check_canonical, the checked mode of ms_ctx_set_checked): which elements of a set of columns store an
// integer >= p.  A read-only streaming kernel: it loads, compares and ORs into a per-lane flag; counting and locating run only in a lane
// whose flag is set, among the few words that lane has just loaded.
//
// Layout.  One launch covers up to MAXCOLS_PER_LAUNCH columns (the pointer table is read in place from the staging ring).  A work item is a
// (tile, column) pair, items are numbered tile-major (item = tile * ncols + column) and workgroup b takes items b, b + G, b + 2G, ...; the
// host picks G <= MAX_GRID as a multiple of ncols whenever ncols <= MAX_GRID, so that a workgroup stays on ONE column and reads its pointer
// once.  The step of the walk is handed in as (dq, dr) = (G / ncols, G % ncols): no division in the loop.
//   Goldilocks (V = 1, 3): the column is a run of n * V words, each tested alone (bad <=> w > 2^64 - 2^32, i.e. high half all ones and low
//     half non-zero).  A tile is TILE_PAIRS 16-byte pairs counted from the 16-byte boundary at or below the column pointer: a column that
//     starts 8 bytes off a boundary has a one-word head (and possibly tail), loaded as single words; everything between goes through
//     16-byte loads, UNROLL of them in flight per lane.  An Fq3 element is counted once, at its first bad component.
//   Fp252 (V = 4): one lane per element, two 16-byte loads (or word / pair / word when the pointer is 8 bytes off); limb 3 decides unless it
//     equals p's, then any non-zero lower limb does.
// Results.  A hit is (count 1, key = column_in_launch * words_per_column + word index of the first bad component): per lane, then folded
// over the workgroup in LDS (sum, min), one Partial per workgroup, and canon_fold reduces those to one -- integer sums and minima only, so
// the answer does not depend on the schedule.  Nothing is ever stored to a column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mscanon {
constexpr int NT = 256;
constexpr int UNROLL = 4;                                  // 16-byte loads in flight per lane
constexpr unsigned TILE_PAIRS = NT * UNROLL;               // Goldilocks tile: 1024 pairs = 16 KiB
constexpr unsigned TILE_ELEMS = NT * (UNROLL / 2);         // Fp252 tile: 512 elements = 16 KiB
constexpr unsigned MAX_GRID = 2048;                        // 256 CUs x 8 workgroups
constexpr unsigned MAXCOLS_PER_LAUNCH = 4096;              // 32 KiB of pointers, read in place (stage_view)
constexpr uint64_t GL_TOP = 0xFFFFFFFF00000000ull;         // p - 1: a word is canonical iff it is <= this
constexpr uint64_t P252_TOP = 0x0800000000000011ull;       // limb 3 of p = 2^251 + 17 * 2^192 + 1 (limbs 0..2: 1, 0, 0)
constexpr uint64_t NONE = ~0ull;

struct alignas(16) W2 { uint64_t a, b; };
struct Partial { uint64_t count, key; };                   // key = NONE when count = 0
struct ScanParams {
    const uint64_t* const* cols;
    Partial* partials;                                     // one per workgroup
    uint64_t nwords;                                       // words per column (n * V)
    uint64_t tiles;                                        // tiles per column
    unsigned ncols, dq, dr;                                // the walk's step G = dq * ncols + dr
};

__host__ __device__ __forceinline__ bool gl_bad(uint64_t w) { return w > GL_TOP; }
__host__ __device__ __forceinline__ bool f252_bad(uint64_t l0, uint64_t l1, uint64_t l2, uint64_t l3) {
    return l3 > P252_TOP || (l3 == P252_TOP && (l0 | l1 | l2) != 0);
}

// sum of counts, minimum of keys over the workgroup -> out[0] (lane 0 writes).  Two levels of sixteen through LDS: three barriers per
// workgroup, once, after its last tile
__device__ inline void block_fold(uint64_t cnt, uint64_t key, Partial* out) {
    __shared__ uint64_t s_cnt[NT];
    __shared__ uint64_t s_key[NT];
    static_assert(NT == 256, "two levels of sixteen");
    const unsigned tid = threadIdx.x;
    s_cnt[tid] = cnt; s_key[tid] = key;
    __syncthreads();
    if (tid < 16) {
        cnt = s_cnt[16 * tid]; key = s_key[16 * tid];
        for (unsigned j = 1; j < 16; j++) { cnt += s_cnt[16 * tid + j]; if (s_key[16 * tid + j] < key) key = s_key[16 * tid + j]; }
        s_cnt[16 * tid] = cnt; s_key[16 * tid] = key;
    }
    __syncthreads();
    if (tid == 0) {
        for (unsigned j = 1; j < 16; j++) { cnt += s_cnt[16 * j]; if (s_key[16 * j] < key) key = s_key[16 * j]; }
        out->count = cnt; out->key = key;
    }
    __syncthreads();                                           // canon_fold aside, nothing follows; keeps the arrays reusable
}

// word `w` of a column of V-word Goldilocks elements is bad: it counts when no earlier component of its element is
template <int V>
__device__ __forceinline__ void gl_hit(const uint64_t* col, uint64_t w, uint64_t key_base, uint64_t& cnt, uint64_t& key) {
    const unsigned k = V == 1 ? 0u : (unsigned)(w % V);
    for (unsigned j = 0; j < k; j++) if (gl_bad(col[w - k + j])) return;
    cnt++;
    if (key_base + w < key) key = key_base + w;
}

template <int V>
__global__ __launch_bounds__(NT) void canon_scan_gl(ScanParams P) {
    const unsigned tid = threadIdx.x;
    uint64_t cnt = 0, key = NONE;
    unsigned c = blockIdx.x % P.ncols, cur = ~0u;
    uint64_t t = blockIdx.x / P.ncols;
    const uint64_t* col = nullptr;
    for (; t < P.tiles; ) {
        if (c != cur) { col = P.cols[c]; cur = c; }
        const unsigned off = (unsigned)(((uintptr_t)col >> 3) & 1);      // words between the 16-byte boundary below and the column
        const W2* base = (const W2*)(col - off);
        const uint64_t end = off + P.nwords;                              // one past the last word, counted from that boundary
        const uint64_t p0 = t * TILE_PAIRS;
        bool bad = false;
        const bool interior = (p0 > 0 || off == 0) && 2 * (p0 + TILE_PAIRS) <= end;
        if (interior) {
            W2 v[UNROLL];
#pragma unroll
            for (int k = 0; k < UNROLL; k++) v[k] = base[p0 + (uint64_t)k * NT + tid];
#pragma unroll
            for (int k = 0; k < UNROLL; k++) bad |= gl_bad(v[k].a) || gl_bad(v[k].b);
        } else {
            for (int k = 0; k < UNROLL; k++) {
                const uint64_t e = 2 * (p0 + (uint64_t)k * NT + tid);
                if (e >= off && e + 1 < end) { const W2 v = base[e >> 1]; bad |= gl_bad(v.a) || gl_bad(v.b); }
                else {
                    if (e >= off && e < end) bad |= gl_bad(col[e - off]);
                    if (e + 1 >= off && e + 1 < end) bad |= gl_bad(col[e + 1 - off]);
                }
            }
        }
        if (bad) {                                                        // this lane's words again, one at a time
            const uint64_t key_base = (uint64_t)c * P.nwords;
            for (int k = 0; k < UNROLL; k++) {
                const uint64_t e = 2 * (p0 + (uint64_t)k * NT + tid);
                for (uint64_t x = e; x < e + 2; x++)
                    if (x >= off && x < end && gl_bad(col[x - off])) gl_hit<V>(col, x - off, key_base, cnt, key);
            }
        }
        c += P.dr; t += P.dq;
        if (c >= P.ncols) { c -= P.ncols; t++; }
    }
    block_fold(cnt, key, P.partials + blockIdx.x);
}

__global__ __launch_bounds__(NT) void canon_scan_252(ScanParams P) {
    const unsigned tid = threadIdx.x;
    constexpr int PER = UNROLL / 2;
    uint64_t cnt = 0, key = NONE;
    unsigned c = blockIdx.x % P.ncols, cur = ~0u;
    uint64_t t = blockIdx.x / P.ncols;
    const uint64_t* col = nullptr;
    const uint64_t n = P.nwords >> 2;
    for (; t < P.tiles; ) {
        if (c != cur) { col = P.cols[c]; cur = c; }
        const bool aligned = (((uintptr_t)col >> 3) & 1) == 0;
        const uint64_t i0 = t * TILE_ELEMS;
        uint64_t l[PER][4];
        bool have[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint64_t i = i0 + (uint64_t)k * NT + tid;
            have[k] = i < n;
            l[k][0] = l[k][1] = l[k][2] = l[k][3] = 0;
            if (!have[k]) continue;
            const uint64_t* e = col + 4 * i;
            if (aligned) {
                const W2 lo = *(const W2*)e, hi = *(const W2*)(e + 2);
                l[k][0] = lo.a; l[k][1] = lo.b; l[k][2] = hi.a; l[k][3] = hi.b;
            } else {
                const W2 mid = *(const W2*)(e + 1);
                l[k][0] = e[0]; l[k][1] = mid.a; l[k][2] = mid.b; l[k][3] = e[3];
            }
        }
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (have[k] && f252_bad(l[k][0], l[k][1], l[k][2], l[k][3])) {
                const uint64_t w = (uint64_t)c * P.nwords + 4 * (i0 + (uint64_t)k * NT + tid);
                cnt++;
                if (w < key) key = w;
            }
        c += P.dr; t += P.dq;
        if (c >= P.ncols) { c -= P.ncols; t++; }
    }
    block_fold(cnt, key, P.partials + blockIdx.x);
}

// one workgroup: the partials of a launch -> out[0]
__global__ __launch_bounds__(NT) void canon_fold(const Partial* parts, unsigned nparts, Partial* out) {
    uint64_t cnt = 0, key = NONE;
    for (unsigned i = threadIdx.x; i < nparts; i += NT) {
        cnt += parts[i].count;
        if (parts[i].key < key) key = parts[i].key;
    }
    block_fold(cnt, key, out);
}
}  // namespace mscanon
