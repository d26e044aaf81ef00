// Starknet's Poseidon over the 252-bit field for gfx950: the Hades permutation with t = 3, S-box x^3, 8 full and 83 partial rounds
// (the Cairo `poseidon` builtin), a sponge over the rows of a matrix and the two-to-one hash of a Merkle node.
//   round r = 0 .. 90:  s[j] += rc[3r + j];  x -> x^3 on all three elements when r < 4 or r >= 87, on s[2] alone otherwise;
//                       mix with M = [[3, 1, 1], [1, -1, 1], [1, 1, -2]]:  t = s0 + s1 + s2,  out = (t + 2 s0, t - 2 s1, t - 3 s2)
//   hash2(x, y)  = permute(x, y, 2)[0]                                            a Merkle node
//   hash_many(v) = append 1, then 0 if the length is odd; from (0, 0, 0): s0 += a, s1 += b, permute, for each pair (a, b); -> s0
// Elements are fp252.h's: four little-endian u64, Montgomery form, and stay in that form throughout -- the constants
// (poseidon252_constants.h, generated) are Montgomery words, and a digest is ONE element of 32 bytes as it lies in a column.
//
// One device `permute` serves the three kernels: a lane per state, a lane per row, a lane per node.  214 products (8 x 3 + 83 cubes of
// a squaring and a product each); everything else runs on fp252.h's lazy forms between canonical points:
//   a_j = s_j + rc_j      s_j, rc_j < p, so a_j < 2p.  An element that is cubed is made canonical first (f252::add: sqr wants a
//                         canonical operand); one that is not (s0, s1 of a partial round) stays lazy (add_lazy).
//   a^3 = mul_t<false>(a, sqr(a))        < 2p: the conditional subtraction is left to the end of the round
//   mix of a0, a1, a2 < 2p               out0 = a0 + a0 + a0 + a1 + a2          <= 10p
//                                        out1 = a0 + a2 + (2p - a1)             <=  6p       (kp_minus<2>, a1 < 2p)
//                                        out2 = a0 + a1 + (4p - (a2 + a2))      <=  8p       (kp_minus<4>, 2 a2 < 4p)
//                         all below 2^256 = 31.9p, the bound of add_lazy and reduce_lazy; reduce_lazy makes the three canonical,
//                         so the state is canonical at every round boundary and every stored word is the reference's.
// The round constants are indexed by the round alone -- the same address in every lane -- and read through a pointer to constant
// global memory, so the compiler fetches them with scalar loads (as the RPO-256 tables are read).  The round loop stays rolled
// (#pragma unroll 1): the body holds six products; unrolling 91 of them is 300 000 instructions.
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "fp252.h"
#include "poseidon252_constants.h"

namespace mspos {

using f252::E;

static constexpr int NT = 256;
static constexpr int MAXCOLS = 128;
static constexpr unsigned TOP = 256;     // parents: the levels of at most this many nodes run in ONE launch of one workgroup (poseidon252_merkle_top)

__device__ __forceinline__ E rc_at(int r, int j) { return E{{RC[r][j][0], RC[r][j][1], RC[r][j][2], RC[r][j][3]}}; }
__device__ __forceinline__ E cube_lazy(const E& a) { return f252::mul_t<false>(a, f252::sqr(a)); }      // canonical a -> a^3 < 2p

// canonical state in, canonical state out
__device__ __forceinline__ void permute(E& s0, E& s1, E& s2) {
    #pragma unroll 1
    for (int r = 0; r < ROUNDS; r++) {
        const bool full = r < FULL_HALF || r >= ROUNDS - FULL_HALF;             // wave-uniform
        E a0, a1;
        if (full) {
            a0 = cube_lazy(f252::add(s0, rc_at(r, 0)));
            a1 = cube_lazy(f252::add(s1, rc_at(r, 1)));
        } else {
            a0 = f252::add_lazy(s0, rc_at(r, 0));
            a1 = f252::add_lazy(s1, rc_at(r, 1));
        }
        const E a2 = cube_lazy(f252::add(s2, rc_at(r, 2)));
        const E t = f252::add_lazy(a0, a2);                                      // < 4p
        s0 = f252::reduce_lazy(f252::add_lazy(f252::add_lazy(t, a1), f252::add_lazy(a0, a0)));
        s1 = f252::reduce_lazy(f252::add_lazy(t, f252::kp_minus<2>(a1)));
        s2 = f252::reduce_lazy(f252::add_lazy(f252::add_lazy(a0, a1), f252::kp_minus<4>(f252::add_lazy(a2, a2))));
    }
}

__device__ __forceinline__ E load_e(const uint64_t* p) { return E{{p[0], p[1], p[2], p[3]}}; }
__device__ __forceinline__ void store_e(uint64_t* p, const E& e) { p[0] = e.l[0]; p[1] = e.l[1]; p[2] = e.l[2]; p[3] = e.l[3]; }

// out[i] = permute(in[i]) over n states of three elements, row-major; out == in is allowed (a lane reads its state before it writes it)
static __global__ void __launch_bounds__(NT) poseidon252_permute(const uint64_t* in, uint64_t* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    E s0 = load_e(in + 12 * i), s1 = load_e(in + 12 * i + 4), s2 = load_e(in + 12 * i + 8);
    permute(s0, s1, s2);
    store_e(out + 12 * i, s0); store_e(out + 12 * i + 4, s1); store_e(out + 12 * i + 8, s2);
}

struct RowsParams {
    const uint64_t* cols[MAXCOLS];
    uint64_t* leaves;        // nrows x 4 words
    size_t nrows;
    unsigned ncols;
    unsigned row_stride;     // elements between rows of one column: 1 (column-major) or ncols (row-major matrix)
};
// leaf[r] = hash_many(row r): one lane per row, the state in registers over the ncols / 2 + 1 absorbs of the row
static __global__ void __launch_bounds__(NT) poseidon252_rows(RowsParams P) {
    const size_t r = (size_t)blockIdx.x * NT + threadIdx.x;
    if (r >= P.nrows) return;
    E s0 = f252::zero(), s1 = f252::zero(), s2 = f252::zero();
    const size_t at = 4 * r * P.row_stride;
    const unsigned npairs = P.ncols / 2 + 1;                                   // the row, a 1, and a 0 when that leaves the length odd
    #pragma unroll 1
    for (unsigned k = 0; k < npairs; k++) {
        const unsigned c0 = 2 * k, c1 = 2 * k + 1;
        if (c0 < P.ncols) s0 = f252::add(s0, load_e(P.cols[c0] + at));
        else s0 = f252::add(s0, f252::one());                                   // c0 == ncols: the padding 1
        if (c1 < P.ncols) s1 = f252::add(s1, load_e(P.cols[c1] + at));
        else if (c1 == P.ncols) s1 = f252::add(s1, f252::one());
        permute(s0, s1, s2);
    }
    store_e(P.leaves + 4 * r, s0);
}

__device__ __forceinline__ E hash2(const uint64_t* pair) {
    E s0 = load_e(pair), s1 = load_e(pair + 4), s2 = E{{TWO[0], TWO[1], TWO[2], TWO[3]}};
    permute(s0, s1, s2);
    return s0;
}
// dst[i] = hash2(src[2i], src[2i+1]) for i < count
static __global__ void __launch_bounds__(NT) poseidon252_merge_level(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, size_t count) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    store_e(dst + 4 * i, hash2(src + 8 * i));
}
// The top of a tree is latency: a level costs one permutation's 182 dependent products however few nodes it has, and lanes cannot
// share a node's partial rounds.  What can be saved is the launches: ONE workgroup of TOP lanes walks every level of at most TOP nodes,
// nodes[k] = hash2(below[2(k - c)], below[2(k - c) + 1]) for k in [c, 2c), c = count, count / 2, .., 1; `src` is the level under the
// first one (the leaves when the tree is that small, otherwise nodes + 4 * 2 * count), every later level reads what the one before
// wrote, with __syncthreads() between them.  That barrier is a workgroup-scope release / acquire: it makes a level's global stores
// visible to the loads of the next level ONLY because both are issued by waves of this ONE workgroup, which sit on one compute unit
// and go through its vector cache in order (the launch is not in threadgroup-split mode).  It orders nothing between workgroups: a
// top spread over several workgroups, or a cooperative one, needs device-scope fences and must not inherit this.
static __global__ void __launch_bounds__(TOP) poseidon252_merkle_top(const uint64_t* src, uint64_t* nodes, unsigned count) {
    const unsigned i = threadIdx.x;
    for (unsigned c = count; c >= 1; c >>= 1) {
        if (i < c) store_e(nodes + 4 * (size_t)(c + i), hash2(src + 8 * (size_t)i));
        __syncthreads();
        src = nodes + 4 * (size_t)c;
    }
}

}  // namespace mspos
