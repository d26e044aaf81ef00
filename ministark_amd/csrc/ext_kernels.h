// Extension columns built in one call (Trace::build_extension_columns, src/trace.rs; examples/brainfuck/trace.rs:108-289): for every
// column e
//     state = init_e;  for row i: out_e[i] = state;  if active_e(i): state = A_e(i) * state + B_e(i)
//     A_e(i) = sum_t sign_t coef_t base[col_t][(i + off_t) mod n],   B_e(i) likewise
// with coef_t a challenge read from device memory (where ms_coin_draw left it) or the literal 1.  The scan is scan_kernels.h's: the maps
// x -> a x + b compose associatively, block aggregate / walk of the aggregates / apply, with its Map, compose, wg_scan and its LDS tile
// crossing.  What differs: a lane's maps are GENERATED from the 8-byte (32-byte) base columns -- one crossing of the tile per term, the
// sums kept in registers -- instead of loaded from materialised a[] / b[] arrays of the extension field, and the columns of a call ride
// gridDim.y, so the call is three launches however many columns it builds.  Every column of a batch has its own terms, so the maps are
// always the general ones (a and b both present; an empty A is the constant 1, an empty B the constant 0).
// All arithmetic is exact field arithmetic: results equal the sequential loop bit for bit.
#pragma once
#include "scan_kernels.h"
#include "table_common.h"

namespace msext {

using msscan::NT;
using msscan::Map;
using msscan::compose;
using msscan::apply;
using msscan::identity;
using msscan::f_zero;
using msscan::wg_scan;
using msscan::Tile;
using msscan::tile_slot;

static constexpr int PER = 4;                 // rows per lane at every length: a workgroup covers ROWS rows
static constexpr int ROWS = NT * PER;
static constexpr int MAXTERMS = 8, MAXEXT = 32;
enum { INIT_ZERO = 0, INIT_ONE = 1, INIT_CHALLENGE = 2 };
using mstab::MASK_ALWAYS;
using mstab::mask_holds;

// resolved on the host: the column's address (nullptr: a constant term), the offset already reduced to [0, n)
struct Term { const uint64_t* col; uint64_t off; int32_t chal; int32_t sign; };      // chal < 0: the literal 1
struct Column {
    Term a[MAXTERMS], b[MAXTERMS];
    const uint64_t* mask;                     // base column of the activity mask (mask_kind != MASK_ALWAYS)
    uint64_t* out;
    uint32_t na, nb;
    int32_t mask_kind, init_kind, init_chal, inclusive;
};
struct Params {
    const Column* cols;                       // [gridDim.y], device memory
    const uint64_t* chal;                     // the challenges: elements of the extension field, Montgomery form
    uint64_t* agg;                            // [ncols][nblocks][2] elements: aggregate map of every block
    uint64_t* block_state;                    // [ncols][nblocks] elements: state at the start of every block
    size_t n;
    unsigned nblocks;
};

// rows [e0, e0 + ROWS) of `src` rotated by off (row i reads src[(i + off) mod n]) -> the lane's PER consecutive rows.  Lanes run along the
// WORDS of the block, as in msscan::load_runs: coalesced whatever the element width (the rotation splits a block's read into at most two
// runs).  Rows past the end read as zero.
template <class B>
__device__ __forceinline__ void load_runs_rot(const uint64_t* __restrict__ src, size_t e0, size_t off, size_t n, uint64_t* tile, typename B::T* out) {
    constexpr int V = B::V, S = PER * V;
    const unsigned t = threadIdx.x;
    #pragma unroll
    for (int j = 0; j < S; j++) {
        const unsigned p = j * NT + t;
        const size_t e = e0 + p / V;
        uint64_t w = 0;
        if (e < n) {
            size_t s = e + off;
            if (s >= n) s -= n;
            w = src[s * V + p % V];
        }
        tile[tile_slot<S>(p)] = w;
    }
    __syncthreads();
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        uint64_t words[V];
        #pragma unroll
        for (int v = 0; v < V; v++) words[v] = tile[tile_slot<S>((t * PER + j) * V + v)];
        out[j] = B::load(words, 0);
    }
    __syncthreads();
}

// acc[j] = sum_t sign_t coef_t base[col_t][row_j + off_t] over the lane's PER rows (nt > 0; the same nt for the whole workgroup)
template <class F, class B>
__device__ __forceinline__ void sum_terms(const Term* terms, unsigned nt, const Params& P, size_t e0, uint64_t* tile, typename F::T* acc) {
    #pragma unroll
    for (int j = 0; j < PER; j++) acc[j] = f_zero<F>();
    for (unsigned k = 0; k < nt; k++) {
        const Term T = terms[k];
        typename F::T c = T.chal >= 0 ? F::load(P.chal, (size_t)T.chal) : F::one();
        if (T.sign < 0) c = F::neg(c);
        if (T.col) {
            typename B::T v[PER];
            load_runs_rot<B>(T.col, e0, T.off, P.n, tile, v);
            #pragma unroll
            for (int j = 0; j < PER; j++) acc[j] = F::add(acc[j], msstage::Mix<F, B>::mul(c, v[j]));
        } else {
            #pragma unroll
            for (int j = 0; j < PER; j++) acc[j] = F::add(acc[j], c);
        }
    }
}

// the PER maps of this lane -> (a[], b[]) in registers and their in-order composition; rows that are masked out or past the end
// are the identity map
template <class F, class B>
__device__ __forceinline__ Map<F> lane_maps(const Params& P, const Column& C, size_t e0, uint64_t* tile, typename F::T* a, typename F::T* b) {
    if (C.na) sum_terms<F, B>(C.a, C.na, P, e0, tile, a);
    if (C.nb) sum_terms<F, B>(C.b, C.nb, P, e0, tile, b);
    const int mask_kind = C.mask_kind;
    typename B::T mk[PER];
    if (mask_kind != MASK_ALWAYS) load_runs_rot<B>(C.mask, e0, 0, P.n, tile, mk);
    Map<F> m = identity<F>();
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        bool active = e0 + (size_t)threadIdx.x * PER + j < P.n;
        if (mask_kind != MASK_ALWAYS) active = active && mask_holds<typename B::T>(mk[j], mask_kind);
        if (!active || !C.na) a[j] = F::one();
        if (!active || !C.nb) b[j] = f_zero<F>();
        const Map<F> mj = {a[j], b[j]};
        m = j ? compose<F, true, true>(m, mj) : mj;
    }
    return m;
}

// grid (nblocks, ncols)
template <class F, class B>
__global__ void __launch_bounds__(NT) ext_reduce(Params P) {
    __shared__ Map<F> sh[NT];
    __shared__ uint64_t tile[Tile<F, PER>::WORDS];
    typename F::T a[PER], b[PER];
    Map<F> m = lane_maps<F, B>(P, P.cols[blockIdx.y], (size_t)blockIdx.x * ROWS, tile, a, b);
    Map<F> excl;
    m = wg_scan<F, true, true>(m, sh, &excl);
    if (threadIdx.x == NT - 1) {
        const size_t k = (size_t)blockIdx.y * P.nblocks + blockIdx.x;
        F::store(P.agg, 2 * k, m.a);
        F::store(P.agg, 2 * k + 1, m.b);
    }
}

// grid (ncols): one workgroup per column, lane t walks blocks [t*chunk, (t+1)*chunk) of its column
template <class F>
__global__ void __launch_bounds__(NT) ext_blocks(Params P) {
    __shared__ Map<F> sh[NT];
    const Column& C = P.cols[blockIdx.x];
    const size_t k0 = (size_t)blockIdx.x * P.nblocks;
    const unsigned chunk = (P.nblocks + NT - 1) / NT;
    const unsigned b0 = threadIdx.x * chunk;
    Map<F> m = identity<F>();
    for (unsigned k = 0; k < chunk; k++) {
        const unsigned blk = b0 + k;
        if (blk < P.nblocks) m = compose<F, true, true>(m, Map<F>{F::load(P.agg, 2 * (k0 + blk)), F::load(P.agg, 2 * (k0 + blk) + 1)});
    }
    Map<F> excl;
    wg_scan<F, true, true>(m, sh, &excl);
    const int init_kind = C.init_kind;
    typename F::T s = init_kind == INIT_CHALLENGE ? F::load(P.chal, (size_t)C.init_chal) : init_kind == INIT_ONE ? F::one() : f_zero<F>();
    s = apply<F, true, true>(excl, s);
    for (unsigned k = 0; k < chunk; k++) {
        const unsigned blk = b0 + k;
        if (blk >= P.nblocks) break;
        F::store(P.block_state, k0 + blk, s);
        s = apply<F, true, true>(Map<F>{F::load(P.agg, 2 * (k0 + blk)), F::load(P.agg, 2 * (k0 + blk) + 1)}, s);
    }
}

// grid (nblocks, ncols)
template <class F, class B>
__global__ void __launch_bounds__(NT) ext_apply(Params P) {
    __shared__ Map<F> sh[NT];
    __shared__ uint64_t tile[Tile<F, PER>::WORDS];
    const Column& C = P.cols[blockIdx.y];
    const size_t e0 = (size_t)blockIdx.x * ROWS;
    typename F::T a[PER], b[PER];
    Map<F> m = lane_maps<F, B>(P, C, e0, tile, a, b);               // the maps stay in registers
    Map<F> excl;
    wg_scan<F, true, true>(m, sh, &excl);
    typename F::T s = apply<F, true, true>(excl, F::load(P.block_state, (size_t)blockIdx.y * P.nblocks + blockIdx.x));
    const bool inclusive = C.inclusive != 0;
    typename F::T out[PER];
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        if (!inclusive) out[j] = s;
        s = apply<F, true, true>(Map<F>{a[j], b[j]}, s);
        if (inclusive) out[j] = s;
    }
    msscan::store_runs<F, PER>(C.out, e0, P.n, tile, out);
}

}  // namespace msext
