// Join rows against a table (include/ministark_hip_join.h): for every row of every key set, the table row that holds its key.
//     first[key] = smallest active table row holding key;   match[s][i] = first[key_s(i)], or NONE for an inactive row or a key not held
// The table is lookup_kernels.h's: mslk::lookup_build, unchanged, over the TABLE side's columns and row count, so the slot array is sized
// by the table and not by the rows joined against it.  What is new is the probe that keeps the row it finds.
//   join_table_active   grid-stride over the table's mask column: the active rows, counted (not launched for an unmasked table)
//   join_match          grid (blocks, sets), grid-stride, one lane per joined row: mask, load_key, hash_key, walk the finished table with
//                       plain loads, same_key against the table side's columns, and ONE coalesced 4-byte store per row, inactive rows
//                       included.  No atomic on the data path.  matched / missing / first accumulate per lane and are reduced through
//                       the wave and the workgroup before they reach device memory: nearly every lane has matched != 0, and one atomic
//                       per lane would be up to 2^20 adds on ONE address (11 ns each) -- per workgroup it is at most 4096.
//                       Integer adds and mins commute: the report is the same on every run; the match array has one writer per entry.
//   join_finish         one lane: the 48-byte report.
// cas / add / amin are table_common.h's (plain read-modify-write under MS_EMU, the HIP atomics otherwise).
#pragma once
#include "lookup_kernels.h"

namespace msjn {

using mslk::NT;
using mslk::MAXW;
using mslk::MAXSETS;
using mslk::EMPTY;
using mslk::Tuple;
using mslk::Key;
using mstab::mask_holds;
using mstab::add;
using mstab::amin;
using mstab::block_totals;

static constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Report { uint64_t matched, missing, first_missing_row; uint32_t first_missing_set, pad; uint64_t duplicate_table_rows, table_active; };
struct Params {
    Tuple table, sets[MAXSETS];               // table: columns of the table side; sets: columns of the probe side
    const uint32_t* slots;                    // [capmask + 1], finished by mslk::lookup_build
    uint32_t* match[MAXSETS];                 // [n] each
    uint64_t* first;                          // min over the missing rows of (set << 32 | row); all ones before join_match
    uint64_t* matched;                        // zero before join_match
    uint64_t* missing;                        // zero before join_match
    uint64_t* dups;                           // zero before lookup_build
    uint64_t* tact;                           // zero before join_table_active
    Report* report;
    size_t n_table, n;
    uint32_t capmask;
    unsigned width;
};

template <int V>
__global__ void __launch_bounds__(NT) join_table_active(Params P) {
    uint64_t act = 0;
    for (size_t j = (size_t)blockIdx.x * NT + threadIdx.x; j < P.n_table; j += (size_t)gridDim.x * NT) act += mask_holds<V>(P.table.mask, P.table.mask_kind, j);
    block_totals(act, 0, ~0ull, P.tact, nullptr, nullptr);
}

// grid (blocks, sets)
template <int V>
__global__ void __launch_bounds__(NT) join_match(Params P) {
    const Tuple& L = P.sets[blockIdx.y];
    uint32_t* const out = P.match[blockIdx.y];
    const unsigned width = P.width;
    uint64_t matched = 0, missing = 0;
    mstab::FirstRow first{~0ull};
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += (size_t)gridDim.x * NT) {
        uint32_t found = NONE;
        if (mask_holds<V>(L.mask, L.mask_kind, i)) {
            const Key<V> k = mslk::load_key<V>(L, width, i);
            uint32_t s = mslk::hash_key<V>(k, width) & P.capmask;
            for (;;) {
                const uint32_t cur = P.slots[s];                       // the table is finished: a plain load
                if (cur == EMPTY) {
                    missing++;
                    first.see(blockIdx.y, i);
                    break;
                }
                if (mslk::same_key<V>(P.table, width, cur, k)) { found = cur; matched++; break; }
                s = (s + 1) & P.capmask;
            }
        }
        out[i] = found;
    }
    block_totals(matched, missing, first.at, P.matched, P.missing, P.first);
}

__global__ void join_finish(Params P) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const mstab::FirstRow first{*P.first};
    Report r;
    r.matched = *P.matched;
    r.missing = *P.missing;
    r.first_missing_row = first.row();
    r.first_missing_set = first.group();
    r.pad = 0;
    r.duplicate_table_rows = *P.dups;
    r.table_active = P.table.mask_kind == mstab::MASK_ALWAYS ? (uint64_t)P.n_table : *P.tact;
    *P.report = r;
}

}  // namespace msjn
