// LogUp lookup columns built in one call (include/ministark_hip_logup.h): for every column e
//     state = init_e;  for row i: out_e[i] = state;  if active_e(i): state = state + sum_f N_f(i) * inv(D_f(i))
//     N_f(i) = sum_t sign_t coef_t base[col_t][(i + off_t) mod n]  (no term: 1),   D_f(i) likewise,   inv(0) = 0
// The increment is a quotient, so the column is a running SUM (the additive forms of scan_kernels.h: compose / apply / wg_scan with
// HAS_A = false) of values that cost an inversion each.  ext_kernels.h recomputes its maps in the apply pass; here that would repeat the
// inversions, so the increments are computed ONCE, stored into the output column itself, and read back by the apply pass:
//   logup_increments  grid (nblocks, ncols): the lane's PER denominators of ONE fraction (sum_terms), inverted by Montgomery's trick in
//                     registers (PER - 1 products, one F::inv, 2 (PER - 1) products back; a zero denominator stays out of the running
//                     product and its inverse is 0, as in msstage::k_batch_inverse), times the numerators, accumulated; fraction after
//                     fraction, so the live set is val[PER] + pre[PER] + acc[PER] whatever nf is.  Increments -> out, block sum -> agg
//   logup_blocks      grid (ncols): one workgroup per column walks the block sums -> the state at the start of every block
//   logup_apply       grid (nblocks, ncols): increments back from out, in-order prefix sum from the block's state, written in place
// All arithmetic is exact field arithmetic: results equal the sequential loop bit for bit.
#pragma once
#include "ext_kernels.h"

namespace mslogup {

using msscan::NT;
using msscan::Map;
using msscan::compose;
using msscan::apply;
using msscan::identity;
using msscan::f_zero;
using msscan::wg_scan;
using msscan::Tile;
using msext::PER;
using msext::ROWS;
using msext::MAXTERMS;
using msext::Term;

static constexpr int MAXFRAC = 4, MAXCOLS = 32;

struct Fraction { Term num[MAXTERMS], den[MAXTERMS]; uint32_t nn, nd; };
struct Column {
    Fraction f[MAXFRAC];
    const uint64_t* mask;                     // base column of the activity mask (mask_kind != MASK_ALWAYS)
    uint64_t* out;
    uint32_t nf;
    int32_t mask_kind, init_kind, init_chal, inclusive;
};
struct Params {
    const Column* cols;                       // [gridDim.y], device memory
    const uint64_t* chal;                     // the challenges: elements of the extension field, Montgomery form
    uint64_t* agg;                            // [ncols][nblocks] elements: sum of the increments of every block
    uint64_t* block_state;                    // [ncols][nblocks] elements: state at the start of every block
    size_t n;
    unsigned nblocks;
};

// grid (nblocks, ncols)
template <class F, class B>
__global__ void __launch_bounds__(NT) logup_increments(Params P) {
    using T = typename F::T;
    __shared__ Map<F> sh[NT];
    __shared__ uint64_t tile[Tile<F, PER>::WORDS];
    const Column& C = P.cols[blockIdx.y];
    const size_t e0 = (size_t)blockIdx.x * ROWS;
    msext::Params E;                          // what sum_terms reads: the challenges and the length
    E.chal = P.chal; E.n = P.n;
    const int mask_kind = C.mask_kind;
    bool active[PER];
    {
        typename B::T mk[PER];
        if (mask_kind != msext::MASK_ALWAYS) msext::load_runs_rot<B>(C.mask, e0, 0, P.n, tile, mk);
        #pragma unroll
        for (int j = 0; j < PER; j++) {
            active[j] = e0 + (size_t)threadIdx.x * PER + j < P.n;
            if (mask_kind != msext::MASK_ALWAYS) active[j] = active[j] && msext::mask_holds<typename B::T>(mk[j], mask_kind);
        }
    }
    T acc[PER];
    #pragma unroll
    for (int j = 0; j < PER; j++) acc[j] = f_zero<F>();
    const unsigned nf = C.nf;
    for (unsigned f = 0; f < nf; f++) {       // the same trip count for the whole workgroup: sum_terms synchronises it
        const Fraction& Q = C.f[f];
        T val[PER], pre[PER];
        msext::sum_terms<F, B>(Q.den, Q.nd, E, e0, tile, val);
        T run = F::one();
        #pragma unroll
        for (int j = 0; j < PER; j++) {
            pre[j] = run;
            if (!active[j]) val[j] = f_zero<F>();                     // masked out or past the end: out of the product, increment zero
            if (!msstage::is_zero<T>(val[j])) run = F::mul(run, val[j]);
        }
        T inv = F::inv(run);
        #pragma unroll
        for (int j = PER - 1; j >= 0; j--) {
            if (!msstage::is_zero<T>(val[j])) {
                const T r = F::mul(inv, pre[j]);
                inv = F::mul(inv, val[j]);
                val[j] = r;
            }                                 // a zero denominator keeps its zero: inv(0) = 0
        }
        if (Q.nn) {
            msext::sum_terms<F, B>(Q.num, Q.nn, E, e0, tile, pre);    // pre[] is free again: the numerators
            #pragma unroll
            for (int j = 0; j < PER; j++) acc[j] = F::add(acc[j], F::mul(pre[j], val[j]));
        } else {
            #pragma unroll
            for (int j = 0; j < PER; j++) acc[j] = F::add(acc[j], val[j]);
        }
    }
    Map<F> m = identity<F>();
    #pragma unroll
    for (int j = 0; j < PER; j++) m.b = F::add(m.b, acc[j]);
    msscan::store_runs<F, PER>(C.out, e0, P.n, tile, acc);
    Map<F> excl;
    m = wg_scan<F, false, true>(m, sh, &excl);
    if (threadIdx.x == NT - 1) F::store(P.agg, (size_t)blockIdx.y * P.nblocks + blockIdx.x, m.b);
}

// grid (ncols): one workgroup per column, lane t walks blocks [t*chunk, (t+1)*chunk) of its column
template <class F>
__global__ void __launch_bounds__(NT) logup_blocks(Params P) {
    __shared__ Map<F> sh[NT];
    const Column& C = P.cols[blockIdx.x];
    const size_t k0 = (size_t)blockIdx.x * P.nblocks;
    const unsigned chunk = (P.nblocks + NT - 1) / NT;
    const unsigned b0 = threadIdx.x * chunk;
    Map<F> m = identity<F>();
    for (unsigned k = 0; k < chunk; k++) {
        const unsigned blk = b0 + k;
        if (blk < P.nblocks) m.b = F::add(m.b, F::load(P.agg, k0 + blk));
    }
    Map<F> excl;
    wg_scan<F, false, true>(m, sh, &excl);
    const int init_kind = C.init_kind;
    typename F::T s = init_kind == msext::INIT_CHALLENGE ? F::load(P.chal, (size_t)C.init_chal) : init_kind == msext::INIT_ONE ? F::one() : f_zero<F>();
    s = apply<F, false, true>(excl, s);
    for (unsigned k = 0; k < chunk; k++) {
        const unsigned blk = b0 + k;
        if (blk >= P.nblocks) break;
        F::store(P.block_state, k0 + blk, s);
        s = F::add(s, F::load(P.agg, k0 + blk));
    }
}

// grid (nblocks, ncols)
template <class F>
__global__ void __launch_bounds__(NT) logup_apply(Params P) {
    __shared__ Map<F> sh[NT];
    __shared__ uint64_t tile[Tile<F, PER>::WORDS];
    const Column& C = P.cols[blockIdx.y];
    const size_t e0 = (size_t)blockIdx.x * ROWS;
    typename F::T b[PER];
    msscan::load_runs<F, PER>(C.out, e0, P.n, tile, b, f_zero<F>());   // the increments logup_increments left there
    Map<F> m = identity<F>();
    #pragma unroll
    for (int j = 0; j < PER; j++) m.b = F::add(m.b, b[j]);
    Map<F> excl;
    wg_scan<F, false, true>(m, sh, &excl);
    typename F::T s = apply<F, false, true>(excl, F::load(P.block_state, (size_t)blockIdx.y * P.nblocks + blockIdx.x));
    const bool inclusive = C.inclusive != 0;
    typename F::T out[PER];
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        if (!inclusive) out[j] = s;
        s = F::add(s, b[j]);
        if (inclusive) out[j] = s;
    }
    msscan::store_runs<F, PER>(C.out, e0, P.n, tile, out);             // in place: the block's increments were read above
}

}  // namespace mslogup
