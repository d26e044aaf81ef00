// What the kernels of the trace-table entry points share (ext_kernels.h, logup_kernels.h, lookup_kernels.h, sort_kernels.h, gap_kernels.h,
// join_kernels.h, direct_count.h):
//   the activity mask   MASK_* and mask_holds: is a row active under (kind, mask column)?  ms_ext.cpp ties the kinds to MS_EXT_*.
//   Canon<V>            the canonical integer of a Montgomery element, least significant word first
//   integer atomics     add / amin / amax / aor / aand / cas / peek: the HIP atomics in the product; under MS_EMU plain read-modify-write,
//                       which is exact there (the simulator runs the lanes of a launch one after another and its header has no 32-bit atomics)
//   FirstRow            the smallest (group << 32 | row) seen -- a report's first missing or overflowing row -- and its decode
//   block_totals        two sums and a minimum of one value per lane -> one add / amin per workgroup
//   block_exclusive     the exclusive prefix of one value per thread of a workgroup, through LDS
//   prefix_in_rounds    the exclusive prefix of an array longer than the workgroup, in place: rounds of one value per thread with a carry
// Everything is inlined into the kernels that use it, which keep their own namespaces and names.
#pragma once
#include "stage_kernels.h"

namespace mstab {

static constexpr int MASK_ALWAYS = 0, MASK_IF_NONZERO = 1, MASK_IF_ZERO = 2;

// is `row` active?  The mask column holds elements of V words; an element is zero when all its words are (Montgomery form keeps zero).
// `mask` and `kind` by reference: a kernel hands in fields of its parameter record, and each is then read where it is needed -- the
// column's address only for a kind that has one
template <int V>
__device__ __forceinline__ bool mask_holds(const uint64_t* const& mask, const int32_t& kind, size_t row) {
    if (kind == MASK_ALWAYS) return true;
    uint64_t any = 0;
    #pragma unroll
    for (int l = 0; l < V; l++) any |= mask[row * V + l];
    return (any == 0) == (kind == MASK_IF_ZERO);
}
// the same on an element already loaded, for a kind that is not MASK_ALWAYS
template <class T>
__device__ __forceinline__ bool mask_holds(const T& v, int kind) { return msstage::is_zero<T>(v) == (kind == MASK_IF_ZERO); }

template <int V> struct Canon;
template <> struct Canon<1> { static __device__ __forceinline__ void words(const uint64_t* col, size_t i, uint64_t* w) { w[0] = gl::from_mont(col[i]); } };
template <> struct Canon<4> {
    static __device__ __forceinline__ void words(const uint64_t* col, size_t i, uint64_t* w) {
        const f252::E c = f252::from_mont(msstage::Fp252T::load(col, i));
        w[0] = c.l[0]; w[1] = c.l[1]; w[2] = c.l[2]; w[3] = c.l[3];
    }
};

#ifdef MS_EMU
static inline uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t o = *p; if (o == expect) *p = v; return o; }
static inline void add(uint32_t* p, uint32_t v) { *p += v; }
static inline void add(uint64_t* p, uint64_t v) { *p += v; }
static inline void amin(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
static inline void amin(uint64_t* p, uint64_t v) { if (v < *p) *p = v; }
static inline void amax(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
static inline void aor(uint64_t* p, uint64_t v) { *p |= v; }
static inline void aand(uint64_t* p, uint64_t v) { *p &= v; }
static inline uint32_t peek(const uint32_t* p) { return *p; }
#else
static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
static __device__ __forceinline__ void add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
static __device__ __forceinline__ void add(uint64_t* p, uint64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
static __device__ __forceinline__ void amin(uint32_t* p, uint32_t v) { atomicMin(p, v); }
static __device__ __forceinline__ void amin(uint64_t* p, uint64_t v) { atomicMin((unsigned long long*)p, (unsigned long long)v); }
static __device__ __forceinline__ void amax(uint64_t* p, uint64_t v) { atomicMax((unsigned long long*)p, (unsigned long long)v); }
static __device__ __forceinline__ void aor(uint64_t* p, uint64_t v) { atomicOr((unsigned long long*)p, (unsigned long long)v); }
static __device__ __forceinline__ void aand(uint64_t* p, uint64_t v) { atomicAnd((unsigned long long*)p, (unsigned long long)v); }
// a slot while other lanes insert: a relaxed load that the compiler neither caches in a register nor serves from the CU's own cache
static __device__ __forceinline__ uint32_t peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// The first row, in (group, row) order, that a report complains of: a lane keeps the smallest it sees, device memory takes the amin over
// the lanes (all ones before the kernel), the finish kernel decodes.  A group is a lookup set or a spec; rows are below 2^32.
struct FirstRow {
    uint64_t at;                                                               // group << 32 | row; all ones: none seen
    __device__ __forceinline__ void see(uint64_t group, uint64_t row) { const uint64_t v = group << 32 | row; if (v < at) at = v; }
    __device__ __forceinline__ uint64_t row() const { return at == ~0ull ? 0 : at & 0xFFFFFFFFull; }
    __device__ __forceinline__ uint32_t group() const { return at == ~0ull ? 0 : (uint32_t)(at >> 32); }
};

// two sums and a minimum of one value per lane -> one add / amin per workgroup, through the wave and LDS; every thread of the workgroup
// calls it.  sum_b and min_lo may be null: nothing is added there.
__device__ __forceinline__ void block_totals(uint64_t a, uint64_t b, uint64_t lo, uint64_t* sum_a, uint64_t* sum_b, uint64_t* min_lo) {
    __shared__ uint64_t s_q[3];
    if (threadIdx.x == 0) { s_q[0] = 0; s_q[1] = 0; s_q[2] = ~0ull; }
    __syncthreads();
#ifndef MS_EMU
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += (uint64_t)__shfl_xor((unsigned long long)a, d);
        b += (uint64_t)__shfl_xor((unsigned long long)b, d);
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)lo, d);
        lo = lo < o ? lo : o;
    }
    const bool speaker = (threadIdx.x & 63u) == 0;
#else
    const bool speaker = true;                                                 // the simulator has no wave: every lane speaks for itself
#endif
    if (speaker) {
        if (a) add(&s_q[0], a);
        if (b) add(&s_q[1], b);
        if (lo != ~0ull) amin(&s_q[2], lo);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_q[0]) add(sum_a, s_q[0]);
        if (sum_b && s_q[1]) add(sum_b, s_q[1]);
        if (min_lo && s_q[2] != ~0ull) amin(min_lo, s_q[2]);
    }
}

// exclusive prefix over the `width` values v of a workgroup (one per thread; width = its thread count), through LDS; every thread calls it
template <class T>
__device__ __forceinline__ T block_exclusive(T v, unsigned width, T* s_a, T* s_b, T* sum) {
    T *in = s_a, *out = s_b;
    in[threadIdx.x] = v;
    __syncthreads();
    for (unsigned d = 1; d < width; d <<= 1) {
        out[threadIdx.x] = in[threadIdx.x] + (threadIdx.x >= d ? in[threadIdx.x - d] : (T)0);
        __syncthreads();
        T* t = in; in = out; out = t;
    }
    const T incl = in[threadIdx.x];
    *sum = in[width - 1];
    __syncthreads();                                                           // the buffers are free again after this
    return incl - v;
}

// a[0 .. count) -> its exclusive prefix, in place, by ONE workgroup of `width` threads: rounds of `width` entries with a carry; -> the total
template <class T>
__device__ __forceinline__ T prefix_in_rounds(T* a, uint32_t count, unsigned width, T* s_a, T* s_b) {
    T carry = 0;
    for (uint32_t base = 0; base < count; base += width) {
        const uint32_t t = base + threadIdx.x;
        const T v = t < count ? a[t] : (T)0;
        T sum;
        const T ex = block_exclusive(v, width, s_a, s_b, &sum);
        if (t < count) a[t] = carry + ex;
        carry += sum;
    }
    return carry;
}

}  // namespace mstab
