// What the kernels of the direct-indexed tables share (range_kernels.h, bitwise_kernels.h): a table whose row index IS the value looked
// up needs no hash table, so both units count into cnt[value] -- in global memory, or in a histogram per workgroup in LDS -- and both
// write columns of small integers next to a report of the rows that did not fit.  Here and nowhere else:
//   NT, LNT, FLUSH_ADDS   the workgroup of a streaming kernel, that of an LDS count, and the adds a lane may make between two flushes
//   above, limb_elem      is an integer above 2^total?  a small integer in Montgomery form
//   hist_words, hist_clear, hist_add, flush_bins   the LDS histogram: 2^HB 32-bit counters (HB <= 15), which cannot overflow, or 2^16 16-bit
//                         counters, two to a word (HB = 16), flushed before a low half can carry into the high one
//   WriterParams, LimbReport, write_limb_report    the parameter record of a kernel that writes columns spec by spec, and its report
// Whatever knows what a bin MEANS -- limbs, operand pairs, op slots -- stays in the unit that defines it.  count_found, from_count, Report
// and EMPTY are lookup_kernels.h's; every atomic is table_common.h's (plain read-modify-write under MS_EMU).
#pragma once
#include "lookup_kernels.h"

namespace msdc {

static constexpr int NT = 256, LNT = 1024;
static constexpr int FLUSH_ADDS = 63;                     // 63 * 1024 = 64 512 adds of a workgroup between two flushes of the packed counters
static_assert(FLUSH_ADDS * LNT <= 65535, "a 16-bit counter must not wrap between two flushes");

using mstab::add;

// is w >> total != 0?  total <= 64 V
template <int V>
__device__ __forceinline__ bool above(const uint64_t* w, unsigned total) {
    uint64_t any = 0;
    #pragma unroll
    for (int l = 0; l < V; l++) {
        const unsigned lo = 64u * l;
        if (total <= lo) any |= w[l];
        else if (total < lo + 64) any |= w[l] >> (total - lo);
    }
    return any != 0;
}

// an integer x < 2^32 in Montgomery form.  Goldilocks: x * 2^64 = x * (2^32 - 1) (mod p), which is below 2^64 -- no general product.
template <class F> __device__ __forceinline__ typename F::T limb_elem(uint32_t x);
template <> __device__ __forceinline__ uint64_t limb_elem<msstage::FpT>(uint32_t x) { return gl::canon(((uint64_t)x << 32) - x); }
template <> __device__ __forceinline__ f252::E limb_elem<msstage::Fp252T>(uint32_t x) { return f252::to_mont(f252::E{{(uint64_t)x, 0, 0, 0}}); }

// ---- the histogram of a workgroup -------------------------------------------------------------------------------------------------
template <int HB> static constexpr unsigned hist_words = HB <= 15 ? 1u << HB : 1u << 15;

// zero before the first add.  Every lane calls it.
__device__ __forceinline__ void hist_clear(uint32_t* hist, unsigned nwords) {
    for (unsigned k = threadIdx.x; k < nwords; k += LNT) hist[k] = 0;
    __syncthreads();
}

template <int HB>
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin) {
    if (HB <= 15) add(hist + bin, 1u);
    else add(hist + (bin >> 1), 1u << (16 * (bin & 1u)));
}

// the histogram -> the global counters: one add per non-zero bin; the histogram is zero again afterwards.  Every lane calls it.
template <int HB>
__device__ __forceinline__ void flush_bins(uint32_t* hist, uint32_t* cnt, unsigned nwords) {
    __syncthreads();
    for (unsigned k = threadIdx.x; k < nwords; k += LNT) {
        const uint32_t w = hist[k];
        if (w == 0) continue;
        hist[k] = 0;
        if (HB <= 15) add(cnt + k, w);
        else {
            if (w & 0xFFFFu) add(cnt + 2 * k, w & 0xFFFFu);
            if (w >> 16) add(cnt + 2 * k + 1, w >> 16);
        }
    }
    __syncthreads();
}

// ---- columns written spec by spec ---------------------------------------------------------------------------------------------------
struct LimbReport { uint64_t overflow, first_overflow_row; uint32_t first_overflow_spec, pad; uint64_t active; };
template <class Spec>
struct WriterParams {
    const Spec* specs;                        // [gridDim.y], device memory
    uint64_t* const* base;                    // the caller's pointer table, device memory
    uint64_t* overflow;                       // zero before the writing kernel
    uint64_t* active;                         // zero
    uint64_t* first;                          // min over the overflowing rows of (spec << 32 | row); all ones
    LimbReport* report;
    size_t n;
};

// one lane, after the writing kernel
template <class Spec>
__device__ __forceinline__ void write_limb_report(const WriterParams<Spec>& P) {
    const mstab::FirstRow first{*P.first};
    LimbReport r;
    r.overflow = *P.overflow;
    r.first_overflow_row = first.row();
    r.first_overflow_spec = first.group();
    r.pad = 0;
    r.active = *P.active;
    *P.report = r;
}

}  // namespace msdc
