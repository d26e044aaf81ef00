// The multiplicity column of a LogUp lookup (include/ministark_hip_lookup.h): how often every table row is looked up.
//     first[key] = smallest active table row holding key;   cnt[first[key_s(i)]] += 1 for every active lookup row i of every set s
// An open-addressing hash table of 32-bit slots (capacity a power of two >= 2 n, so the load factor is at most 1/2 and a probe walk always
// ends), linear probing, wrapping at the capacity.  A slot holds a table ROW INDEX and nothing else; EMPTY = 0xFFFFFFFF.  The keys stay where
// they are, in the input columns, which no kernel of the call writes.
//   lookup_build    grid-stride, one lane per table row: hash the tuple's words, walk from the hashed slot.  Empty slot: compare-and-swap
//                   the row index in (lost the race: go on with the value that won).  Occupied slot: compare the keys -- equal: atomicMin
//                   the slot with the own index and count a duplicate; unequal: next slot.
//                   Whatever the order of the inserts, a key ends in exactly one slot (a later row of the same key finds it before any empty
//                   slot, since slots never empty again), that slot ends as the MINIMUM of the key's rows, and every row of a key but the one
//                   whose compare-and-swap created the slot counts one duplicate: rows - 1 per key.  WHICH slot a key takes depends on the
//                   order; nothing that leaves the call does.
//   lookup_count    grid (blocks, sets), grid-stride, one lane per lookup row: the same walk over the finished table.  Found: atomicAdd on the
//                   32-bit counter of the row found (one add per wave for the lanes that found the same row: count_found).  Empty slot: the
//                   tuple is missing -- counted, and atomicMin on (set << 32 | row).
//                   Integer adds and mins commute: the counters and the report are the same on every run.
//   lookup_finish   grid-stride: counter -> field element in Montgomery form -> d_m; lane 0 writes the report.
// The mask predicate and cas / add / amin / peek are table_common.h's (plain read-modify-write under MS_EMU, the HIP atomics otherwise).
#pragma once
#include "table_common.h"

namespace mslk {

static constexpr int NT = 256, MAXW = 4, MAXSETS = 8;
static constexpr uint32_t EMPTY = 0xFFFFFFFFu;

using mstab::mask_holds;
using mstab::cas;
using mstab::amin;
using mstab::add;
using mstab::peek;

struct Tuple {
    const uint64_t* cols[MAXW];               // cols[0 .. width)
    const uint64_t* mask;                     // base column of the activity mask (mask_kind != MASK_ALWAYS)
    int32_t mask_kind, pad;
};
struct Report { uint64_t missing, first_missing_row; uint32_t first_missing_set, pad; uint64_t duplicate_table_rows; };
struct Params {
    Tuple table, sets[MAXSETS];
    uint32_t* slots;                          // [capmask + 1], EMPTY before lookup_build
    uint32_t* cnt;                            // [n], zero before lookup_count
    uint64_t* first;                          // min over the missing tuples of (set << 32 | row); all ones before lookup_count
    uint64_t* missing;                        // zero before lookup_count
    uint64_t* dups;                           // zero before lookup_build
    uint64_t* m;
    Report* report;
    size_t n;
    uint32_t capmask;
    unsigned width;
};

template <int V> struct Key { uint64_t w[MAXW * V]; };

// the words of row i's tuple; components past the width are zero (in the key and in every key it is compared with)
template <int V>
__device__ __forceinline__ Key<V> load_key(const Tuple& T, unsigned width, size_t i) {
    Key<V> k;
    #pragma unroll
    for (int c = 0; c < MAXW; c++) {
        #pragma unroll
        for (int l = 0; l < V; l++) k.w[c * V + l] = (unsigned)c < width ? T.cols[c][i * V + l] : 0;
    }
    return k;
}

template <int V>
__device__ __forceinline__ bool same_key(const Tuple& T, unsigned width, size_t j, const Key<V>& k) {
    uint64_t diff = 0;
    #pragma unroll
    for (int c = 0; c < MAXW; c++) {
        #pragma unroll
        for (int l = 0; l < V; l++) if ((unsigned)c < width) diff |= T.cols[c][j * V + l] ^ k.w[c * V + l];
    }
    return diff == 0;
}

// Every word goes through a multiply and a fold of the high half into the low: keys 0 .. n-1 (Montgomery form: multiples of one constant)
// and keys that differ in one limb of one component spread over the slots like random ones.  The constants are splitmix64's.
template <int V>
__device__ __forceinline__ uint32_t hash_key(const Key<V>& k, unsigned width) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    #pragma unroll
    for (int c = 0; c < MAXW; c++) {
        #pragma unroll
        for (int l = 0; l < V; l++)
            if ((unsigned)c < width) { h = (h ^ k.w[c * V + l]) * 0xBF58476D1CE4E5B9ull; h ^= h >> 29; }
    }
    h *= 0x94D049BB133111EBull;
    h ^= h >> 32;
    return (uint32_t)h;
}

template <int V>
__global__ void __launch_bounds__(NT) lookup_build(Params P) {
    const Tuple& T = P.table;
    const unsigned width = P.width;
    uint64_t dups = 0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += (size_t)gridDim.x * NT) {
        if (!mask_holds<V>(T.mask, T.mask_kind, i)) continue;
        const Key<V> k = load_key<V>(T, width, i);
        uint32_t s = hash_key<V>(k, width) & P.capmask;
        for (;;) {
            uint32_t cur = peek(P.slots + s);
            // The compare-and-swap publishes a row INDEX only.  What a reader of the slot goes on to read -- the key -- lies in the input
            // columns, written before the call and by none of its kernels: there is no payload to order after the index, so no fence.
            if (cur == EMPTY) cur = cas(P.slots + s, EMPTY, (uint32_t)i);
            if (cur == EMPTY) break;                                   // the slot was empty and is this row's now
            // `cur` may be lowered by an atomicMin meanwhile, but only to another row of the SAME key: the comparison holds either way
            if (same_key<V>(T, width, cur, k)) { amin(P.slots + s, (uint32_t)i); dups++; break; }
            s = (s + 1) & P.capmask;
        }
    }
    if (dups) add(P.dups, dups);
}

// One atomicAdd for all the lanes of a wave that found the row the wave's first finder found, one each for the others.  Every lookup hitting
// ONE table row is the shape of padding rows: n adds to one address take 11 ns each, 64 times fewer do not.  One round only:
// on spread-out lookups the leader's group is the leader alone and the cost is two ballots and a lane read per row.  Correct for any set
// of lanes that gets here together -- the ballots count exactly the lanes that execute them.  Wave-level builtins are identities in the
// simulator, which therefore takes the plain form (as the product does with AGG = false, kept for scripts/lookup_probe.py).
template <bool AGG>
__device__ __forceinline__ void count_found(uint32_t* cnt, uint32_t found) {
#ifndef MS_EMU
    if (AGG) {
        const bool has = found != EMPTY;
        const unsigned long long todo = __ballot(has);
        if (todo == 0) return;
        const int src = __builtin_amdgcn_readfirstlane((int)__ffsll(todo) - 1);
        const uint32_t lead = __builtin_amdgcn_readlane(found, src);
        const unsigned long long same = __ballot(has && found == lead);
        if (has && found != lead) add(cnt + found, 1u);
        else if (has && (int)(threadIdx.x & 63u) == (int)__ffsll(same) - 1) add(cnt + lead, (uint32_t)__popcll(same));
        return;
    }
#endif
    if (found != EMPTY) add(cnt + found, 1u);
}

// grid (blocks, sets)
template <int V, bool AGG>
__global__ void __launch_bounds__(NT) lookup_count(Params P) {
    const Tuple& L = P.sets[blockIdx.y];
    const unsigned width = P.width;
    uint64_t missing = 0;
    mstab::FirstRow first{~0ull};
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += (size_t)gridDim.x * NT) {
        uint32_t found = EMPTY;
        if (mask_holds<V>(L.mask, L.mask_kind, i)) {
            const Key<V> k = load_key<V>(L, width, i);
            uint32_t s = hash_key<V>(k, width) & P.capmask;
            for (;;) {
                const uint32_t cur = P.slots[s];
                if (cur == EMPTY) {
                    missing++;
                    first.see(blockIdx.y, i);
                    break;
                }
                if (same_key<V>(P.table, width, cur, k)) { found = cur; break; }
                s = (s + 1) & P.capmask;
            }
        }
        count_found<AGG>(P.cnt, found);
    }
    if (missing) { add(P.missing, missing); amin(P.first, first.at); }
}

template <class F> __device__ __forceinline__ typename F::T from_count(uint32_t c);
template <> __device__ __forceinline__ uint64_t from_count<msstage::FpT>(uint32_t c) { return gl::to_mont((uint64_t)c); }
template <> __device__ __forceinline__ f252::E from_count<msstage::Fp252T>(uint32_t c) { return c ? f252::to_mont(f252::E{{(uint64_t)c, 0, 0, 0}}) : f252::zero(); }

// one lane of a finish kernel: the report of a count, from its `missing` and the amin over the missing rows of (set << 32 | row)
__device__ __forceinline__ void write_report(Report* report, uint64_t missing, uint64_t first_at, uint64_t dups) {
    const mstab::FirstRow first{first_at};
    Report r;
    r.missing = missing;
    r.first_missing_row = first.row();
    r.first_missing_set = first.group();
    r.pad = 0;
    r.duplicate_table_rows = dups;
    *report = r;
}

template <class F>
__global__ void __launch_bounds__(NT) lookup_finish(Params P) {
    for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < P.n; j += (size_t)gridDim.x * NT) F::store(P.m, j, from_count<F>(P.cnt[j]));
    if (blockIdx.x == 0 && threadIdx.x == 0) write_report(P.report, *P.missing, *P.first, *P.dups);
}

}  // namespace mslk
