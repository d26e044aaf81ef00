// A stable multi-column key sort of trace rows and a gather by a device-resident index (include/ministark_hip_sort.h).
//     perm = sorted(active rows, key = the canonical integers of the key's columns, cols[0] most significant) + inactive rows
// A least-significant-digit radix sort, radix 256, over the canonical words of the key: word W = (nkeys - 1 - k) * V + l is limb l of
// component k, digit position 8 W + b its byte b, so ascending positions are ascending significance.  Nothing goes back to the host: a
// one-thread launch writes a Table that tells every later launch whether its position is skipped and which of the two ping-pong buffers is
// its source.  No workgroup waits on another: whatever one launch needs from all workgroups of an earlier one is a launch boundary away.
//   sort_prepare   grid-stride: evaluates the mask (flag[i] = 1 for an inactive row), writes the identity into perm[0], converts every key
//                  component out of Montgomery form into keys[W][i], and reduces the OR and the AND of every word over the active rows
//                  (registers -> wave -> LDS -> one atomic per word and workgroup).  A bit takes one value on all active rows exactly when
//                  OR and AND agree on it: byte b of word W varies iff byte b of OR ^ AND is not zero.  Integer or/and/add commute: the same
//                  on every run.
//   sort_decide    one thread: the Table and the report.  A position is skipped when its byte does not vary; the flag pass (the stable
//                  partition active | inactive, a pass with two bins over all n rows) when no row or every row is active.  Every executed
//                  pass flips the buffer parity.
//   sort_gather    per word with a varying byte: kw[par][i] = keys[W][perm[par][i]] for i < active -- one random read per word, after which
//                  the word's passes stream (word, index) pairs.
//   pass_hist      per tile of T rows: the 256 digit counts (LDS integer atomics) -> hist[digit][tile]
//   pass_scan      one workgroup per digit: the exclusive prefix of hist[digit][*] in place, in rounds of SCAN_ROUND tiles with a carry (of
//                  64 or 128 threads when there are no more tiles than that), and total[digit]
//   pass_scatter   per tile: the exclusive prefix of total[] (the digit's first slot), plus hist[digit][tile] (the slots of earlier tiles),
//                  plus the rank of the row among the rows of its digit in the tile, IN ROW ORDER -- that is what makes the pass stable.
//                  Wave w of a tile takes rows [512 w, 512 w + 512) in eight rounds of 64 consecutive rows.  In a round, eight ballots (one
//                  per digit bit) give every lane the set of lanes that hold its digit: the lanes below it are its rank in the round, and
//                  the lowest lane of each set adds the set's size to the wave's running count of that digit in LDS, read by all before.
//                  No atomic hands out a rank, so arrival order never enters.  After the rounds the counts of the waves before are added.
//                  Under MS_EMU the wave builtins are identities and the lanes run one after another: a barrier per round puts the threads
//                  of a wave in (round, lane) order and the rank is the running count itself.
//   sort_finish    perm[0] IS d_perm: copies from perm[1] the sorted head when the final parity is 1, and the inactive tail, which no key
//                  pass moves, when the flag pass ran
//   permute_columns  dst[c][i] = src[c][index[i]], zero for index[i] >= n_src
#pragma once
#include "table_common.h"

namespace mssort {

static constexpr int NT = 256, MAXK = 4, ITEMS = 8, TILE = NT * ITEMS, WAVES = NT / 64, WAVE_ROWS = 64 * ITEMS, SCAN_ROUND = NT;
static constexpr int MAXWORDS = MAXK * 4, MAXPOS = MAXWORDS * 8, PREPARE_MAX_GRID = 1024, MAXCOLS = 128;
static constexpr uint32_t FLAG_POS = 0xFFFFFFFFu;
using mstab::MASK_ALWAYS;
using mstab::mask_holds;
using mstab::Canon;
using mstab::add;
using mstab::aor;
using mstab::aand;
using mstab::block_exclusive;

struct Report { uint64_t active, varying_bytes; };
struct Table {
    uint32_t active, final_par, flag_skip, pad;
    uint8_t skip[MAXPOS], src[MAXPOS];        // per digit position: not executed; the parity of its source buffers
    uint8_t wskip[MAXWORDS], wsrc[MAXWORDS];  // per word: no byte varies; the parity its gather reads perm from and writes kw to
};
struct Params {
    const uint64_t* cols[MAXK];               // cols[0 .. nkeys), Montgomery form
    const uint64_t* mask;                     // mask_kind != MASK_ALWAYS
    uint64_t* keys;                           // [nwords][n] canonical words
    uint64_t* kw[2];                          // [n] the current word in the current order
    uint32_t* perm[2];                        // perm[0] = d_perm
    uint8_t* flag;                            // [n], mask_kind != MASK_ALWAYS
    uint32_t* hist;                           // [256][ntiles]
    uint32_t* total;                          // [256]
    uint64_t* red;                            // [0] active rows, [1 + W] OR of word W, [1 + MAXWORDS + W] AND of word W
    Table* tab;
    Report* report;
    uint32_t n, ntiles, nkeys, nwords;
    int32_t mask_kind, pad;
};

template <int V>
__global__ void __launch_bounds__(NT) sort_prepare(Params P) {
    __shared__ uint64_t s_or[MAXWORDS], s_and[MAXWORDS];
    __shared__ uint32_t s_active;
    uint64_t vor[MAXK * V], vand[MAXK * V];
    #pragma unroll
    for (int w = 0; w < MAXK * V; w++) { vor[w] = 0; vand[w] = ~0ull; }
    uint32_t nact = 0;
    if (threadIdx.x < MAXWORDS) { s_or[threadIdx.x] = 0; s_and[threadIdx.x] = ~0ull; }
    if (threadIdx.x == 0) s_active = 0;
    __syncthreads();
    const size_t n = P.n;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        const bool act = mask_holds<V>(P.mask, P.mask_kind, i);
        if (P.flag) P.flag[i] = act ? 0 : 1;
        P.perm[0][i] = (uint32_t)i;
        nact += act;
        #pragma unroll
        for (int k = 0; k < MAXK; k++) {
            if ((unsigned)k < P.nkeys) {
                uint64_t w[V];
                Canon<V>::words(P.cols[k], i, w);
                const size_t W0 = (size_t)(P.nkeys - 1 - k) * V;
                #pragma unroll
                for (int l = 0; l < V; l++) {
                    P.keys[(W0 + l) * n + i] = w[l];
                    if (act) { vor[k * V + l] |= w[l]; vand[k * V + l] &= w[l]; }
                }
            }
        }
    }
#ifndef MS_EMU
    #pragma unroll
    for (int w = 0; w < MAXK * V; w++) {
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            vor[w] |= (uint64_t)__shfl_xor((unsigned long long)vor[w], d);
            vand[w] &= (uint64_t)__shfl_xor((unsigned long long)vand[w], d);
        }
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nact += __shfl_xor(nact, d);
    const bool speaker = (threadIdx.x & 63u) == 0;
#else
    const bool speaker = true;
#endif
    if (speaker) {
        #pragma unroll
        for (int k = 0; k < MAXK; k++) {
            if ((unsigned)k < P.nkeys) {
                #pragma unroll
                for (int l = 0; l < V; l++) { aor(&s_or[k * V + l], vor[k * V + l]); aand(&s_and[k * V + l], vand[k * V + l]); }
            }
        }
        add(&s_active, nact);
    }
    __syncthreads();
    // register slot k V + l is word (nkeys - 1 - k) V + l
    if (threadIdx.x < P.nkeys * V) {
        const unsigned k = threadIdx.x / V, l = threadIdx.x % V, W = (P.nkeys - 1 - k) * V + l;
        aor(P.red + 1 + W, s_or[threadIdx.x]);
        aand(P.red + 1 + MAXWORDS + W, s_and[threadIdx.x]);
    }
    if (threadIdx.x == 0 && s_active) add(P.red, (uint64_t)s_active);
}

__global__ void __launch_bounds__(64) sort_decide(Params P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Table& T = *P.tab;
    const uint32_t A = (uint32_t)P.red[0];
    uint32_t par = 0;
    uint64_t varying = 0;
    const bool flag_skip = P.mask_kind == MASK_ALWAYS || A == 0 || A == P.n;
    if (!flag_skip) par ^= 1;
    for (uint32_t W = 0; W < P.nwords; W++) {
        const uint64_t diff = A ? (P.red[1 + W] ^ P.red[1 + MAXWORDS + W]) : 0;
        T.wsrc[W] = (uint8_t)par;
        T.wskip[W] = diff == 0;
        for (uint32_t b = 0; b < 8; b++) {
            const bool v = ((diff >> (8 * b)) & 0xFF) != 0;
            T.skip[W * 8 + b] = !v;
            T.src[W * 8 + b] = (uint8_t)par;
            if (v) { par ^= 1; varying++; }
        }
    }
    T.active = A; T.final_par = par; T.flag_skip = flag_skip; T.pad = 0;
    Report r;
    r.active = A; r.varying_bytes = varying;
    *P.report = r;
}

__global__ void __launch_bounds__(NT) sort_gather(Params P, uint32_t W) {
    const Table& T = *P.tab;
    if (T.wskip[W]) return;
    const uint32_t par = T.wsrc[W], cnt = T.active;
    const uint64_t* key = P.keys + (size_t)W * P.n;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < cnt; i += (size_t)gridDim.x * NT) P.kw[par][i] = key[P.perm[par][i]];
}

// what a launch of a pass needs from the table: is it executed, its source parity, how many rows it orders
struct Pass { bool skip; uint32_t par, cnt; };
__device__ __forceinline__ Pass pass_of(const Params& P, uint32_t pos) {
    const Table& T = *P.tab;
    if (pos == FLAG_POS) return Pass{T.flag_skip != 0, 0u, P.n};
    return Pass{T.skip[pos] != 0, (uint32_t)T.src[pos], T.active};
}
// the digit of the row at place i of the source order (the flag pass orders the identity: the row IS i)
__device__ __forceinline__ uint32_t digit_at(const Params& P, uint32_t pos, uint32_t par, size_t i) {
    if (pos == FLAG_POS) return P.flag[i];
    return (uint32_t)(P.kw[par][i] >> (8 * (pos & 7))) & 0xFFu;
}
// place of (wave, round, lane) in the tile: a wave's rows are consecutive, a round's 64 rows too
__device__ __forceinline__ size_t place(uint32_t tile, uint32_t j) {
    return (size_t)tile * TILE + (threadIdx.x >> 6) * WAVE_ROWS + j * 64 + (threadIdx.x & 63u);
}

__global__ void __launch_bounds__(NT) pass_hist(Params P, uint32_t pos) {
    const Pass ps = pass_of(P, pos);
    if (ps.skip) return;
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    if ((size_t)blockIdx.x * TILE < ps.cnt) {
        #pragma unroll
        for (int j = 0; j < ITEMS; j++) {
            const size_t i = place(blockIdx.x, j);
            if (i < ps.cnt) add(&s_hist[digit_at(P, pos, ps.par, i)], 1u);
        }
    }
    __syncthreads();
    P.hist[(size_t)threadIdx.x * P.ntiles + blockIdx.x] = s_hist[threadIdx.x];
}

// grid: 256 workgroups, one per digit, of scan_threads(ntiles) threads: a round takes as many tiles
__host__ __device__ inline unsigned scan_threads(uint32_t ntiles) { return ntiles <= 64 ? 64u : ntiles <= 128 ? 128u : (unsigned)SCAN_ROUND; }
__global__ void __launch_bounds__(NT) pass_scan(Params P, uint32_t pos) {
    const Pass ps = pass_of(P, pos);
    if (ps.skip) return;
    __shared__ uint32_t s_a[NT], s_b[NT];
    const uint32_t carry = mstab::prefix_in_rounds(P.hist + (size_t)blockIdx.x * P.ntiles, P.ntiles, blockDim.x, s_a, s_b);
    if (threadIdx.x == 0) P.total[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(NT) pass_scatter(Params P, uint32_t pos) {
    const Pass ps = pass_of(P, pos);
    if (ps.skip) return;
    if ((size_t)blockIdx.x * TILE >= ps.cnt) return;
    __shared__ uint32_t s_a[NT], s_b[NT];
    __shared__ uint32_t s_cnt[WAVES][256];                                     // per wave and digit: rows so far, then the slot of the wave's first
    const uint32_t wave = threadIdx.x >> 6;
    #pragma unroll
    for (int w = 0; w < WAVES; w++) s_cnt[w][threadIdx.x] = 0;
    uint32_t sum;
    const uint32_t first = block_exclusive(P.total[threadIdx.x], blockDim.x, s_a, s_b, &sum)                  // the barriers in it publish the zeros too
                           + P.hist[(size_t)threadIdx.x * P.ntiles + blockIdx.x];
    uint32_t dig[ITEMS], rank[ITEMS];
    #pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const size_t i = place(blockIdx.x, j);
        const bool valid = i < ps.cnt;
        const uint32_t d = valid ? digit_at(P, pos, ps.par, i) : 0u;
        dig[j] = d;
#ifdef MS_EMU
        rank[j] = 0;
        if (valid) { rank[j] = s_cnt[wave][d]; s_cnt[wave][d] = rank[j] + 1; }
        __syncthreads();
#else
        unsigned long long same = __ballot(valid);
        #pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t before = valid ? s_cnt[wave][d] : 0u;
        __builtin_amdgcn_wave_barrier();                                       // every lane has read before the set's lowest lane writes
        rank[j] = before + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && lane == (uint32_t)__ffsll((long long)same) - 1u) s_cnt[wave][d] = before + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
#endif
    }
    __syncthreads();
    {   // thread d: the slot of each wave's first row of digit d
        uint32_t at = first;
        #pragma unroll
        for (int w = 0; w < WAVES; w++) { const uint32_t c = s_cnt[w][threadIdx.x]; s_cnt[w][threadIdx.x] = at; at += c; }
    }
    __syncthreads();
    const uint32_t q = ps.par ^ 1u;
    #pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const size_t i = place(blockIdx.x, j);
        if (i < ps.cnt) {
            const uint32_t to = s_cnt[wave][dig[j]] + rank[j];
            P.perm[q][to] = P.perm[ps.par][i];
            if (pos != FLAG_POS) P.kw[q][to] = P.kw[ps.par][i];
        }
    }
}

__global__ void __launch_bounds__(NT) sort_finish(Params P) {
    // the key passes move the active head only: the inactive tail lies where the flag pass put it
    const uint32_t head = P.tab->final_par, tail = P.tab->flag_skip ? 0u : 1u, A = P.tab->active;
    if (head == 0 && tail == 0) return;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += (size_t)gridDim.x * NT)
        if ((i < A ? head : tail) == 1) P.perm[0][i] = P.perm[1][i];
}

struct PermuteParams {
    const uint64_t* src[MAXCOLS];
    uint64_t* dst[MAXCOLS];
    const uint32_t* index;
    size_t n_src, n_out;
};
// grid (blocks, columns)
template <int V>
__global__ void __launch_bounds__(NT) permute_columns(PermuteParams P) {
    const uint64_t* src = P.src[blockIdx.y];
    uint64_t* dst = P.dst[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n_out; i += (size_t)gridDim.x * NT) {
        const size_t from = P.index[i];
        const bool in = from < P.n_src;
        #pragma unroll
        for (int l = 0; l < V; l++) dst[i * V + l] = in ? src[from * V + l] : 0ull;
    }
}

}  // namespace mssort
