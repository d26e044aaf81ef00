// The Poseidon public coin of the 252-bit field: an algebraic Fiat-Shamir transcript with its state resident on the device
// (ms_hades_coin_* of include/ministark_hip_hades_coin.h).  The coin is NOT a sponge: Hades has t = 3, a lone lane pays a whole
// permutation's 182 dependent products, and a sponge squeezing two elements a permutation would chain ten or twenty of them for the
// DEEP coefficients alone.  It keeps ONE field element and a draw counter, as mscoin::coin_step's byte coins keep (seed, counter):
// absorbing is serial, every draw of a call is an independent permutation (one lane each, one permutation's latency whatever the
// count), and the proof-of-work search is the same shape at full width.
//
// State (ms_hades_coin_state, 56 bytes in HBM): digest = one element in Montgomery form, n_draws, four zero pad words.  The rules (the
// project's own), on mspos::permute / hash2 / hash_many of poseidon252_kernels.h:
//   create          digest = seed; n_draws = 0                                    (the host writes the record; no permutation)
//   reseed_digest   digest = hash2(digest, d); n_draws = 0                        hash2(x, y) = permute(x, y, 2)[0], the Merkle node
//   reseed_int      digest = hash2(digest, v); n_draws = 0                        v any u64
//   reseed_elements digest = hash2(digest, hash_many(e)); n_draws = 0
//   draw            out[i] = permute(digest, n_draws + i, 3)[0], i < count; n_draws += count
//   queries         (draw as a canonical integer) & (domain_size - 1)
//   grind           nonce n is accepted when permute(digest, n, 4)[0], as a canonical integer, has its low `bits` bits zero
// The third state element is the domain tag -- 2 absorb, 3 draw, 4 proof-of-work -- so that reseed_int(v) never produces what draw
// number v published, and the digest after reseed_int(nonce) is another permutation's output than the one the search tested.
// Everything goes through mspos::permute, so every word is the reference's; the constants are read as poseidon252_kernels.h reads them.
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "fp252.h"
#include "poseidon252_kernels.h"

namespace mshades {

using f252::E;

static constexpr int NT = 256;                  // draws and the proof-of-work search: one permutation per lane

// the device image of ms_hades_coin_state
struct State {
    uint64_t digest[4];
    uint64_t n_draws;
    uint32_t pad[4];
};
static_assert(sizeof(State) == 56, "ms_hades_coin_state is 56 bytes");

__device__ __forceinline__ E small(uint64_t v) { return f252::to_mont(E{{v, 0, 0, 0}}); }                     // any u64 is below p
__device__ __forceinline__ E tag_absorb() { return E{{mspos::TWO[0], mspos::TWO[1], mspos::TWO[2], mspos::TWO[3]}}; }
__device__ __forceinline__ E tag_draw() { return f252::add(tag_absorb(), f252::one()); }                       // 3
__device__ __forceinline__ E tag_pow() { return f252::add(tag_absorb(), tag_absorb()); }                       // 4

enum { OP_RESEED_DIGEST = 0, OP_RESEED_INT = 1, OP_RESEED_ELEMENTS = 2 };

// The chain: one lane, one launch for a whole reseed.  `in`: the element of reseed_digest, or `count` >= 1 elements of
// reseed_elements; `arg`: the integer of reseed_int.  The hash_many pairs (the elements, a 1, and a 0 when that leaves the length
// odd: count / 2 + 1 permutations from the zero state) and the closing hash2 run through ONE rolled loop around one inlined
// mspos::permute, the state in registers throughout; the record is loaded once and stored once.  Nothing here depends on a lane
// index, so the compiler proves every value wave-uniform and runs the chain on the scalar unit (the stores stay vector stores):
// 253 us a permutation against the 226 of a lone vector lane.
static __global__ void __launch_bounds__(64) hades_coin_absorb(State* coin, const uint64_t* __restrict__ in, uint64_t arg, size_t count, int op) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const E digest = mspos::load_e(coin->digest);
    E s0 = f252::zero(), s1 = f252::zero(), s2 = f252::zero();
    size_t npairs = 0;
    if (op == OP_RESEED_DIGEST) s0 = mspos::load_e(in);
    else if (op == OP_RESEED_INT) s0 = small(arg);
    else npairs = count / 2 + 1;
    #pragma unroll 1
    for (size_t k = 0; k <= npairs; k++) {
        if (k < npairs) {
            const size_t c0 = 2 * k, c1 = 2 * k + 1;
            if (c0 < count) s0 = f252::add(s0, mspos::load_e(in + 4 * c0));
            else s0 = f252::add(s0, f252::one());                               // c0 == count: the padding 1
            if (c1 < count) s1 = f252::add(s1, mspos::load_e(in + 4 * c1));
            else if (c1 == count) s1 = f252::add(s1, f252::one());
        } else {                                                                // the closing hash2(digest, what was absorbed)
            s1 = s0;
            s0 = digest;
            s2 = tag_absorb();
        }
        mspos::permute(s0, s1, s2);
    }
    mspos::store_e(coin->digest, s0);
    coin->n_draws = 0;
}

// One lane per output: out[i] = permute(digest, n_draws + i, 3)[0], the counter turned into Montgomery form in the lane.  With
// `queries` the output is one u64 per draw, (the element as an integer) & qmask.  n_draws advances in exactly one lane, after every
// lane that reads the record has read it: a grid of ONE workgroup does it here, behind the barrier (`bump`); a longer draw leaves
// the record alone and the host enqueues hades_coin_advance behind it on the same stream -- workgroups of one grid have no order.
static __global__ void __launch_bounds__(NT) hades_coin_draw(State* coin, size_t count, uint64_t* __restrict__ out, uint64_t qmask, int queries, int bump) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    E s0 = mspos::load_e(coin->digest);
    const uint64_t first = coin->n_draws;
    if (bump) {
        __syncthreads();
        if (threadIdx.x == 0) coin->n_draws = first + count;
    }
    if (i >= count) return;
    E s1 = small(first + i), s2 = tag_draw();
    mspos::permute(s0, s1, s2);
    if (queries) out[i] = f252::from_mont(s0).l[0] & qmask;
    else mspos::store_e(out + 4 * i, s0);
}
static __global__ void __launch_bounds__(64) hades_coin_advance(State* coin, uint64_t count) {
    if (threadIdx.x == 0 && blockIdx.x == 0) coin->n_draws += count;
}

// One nonce per lane, the digest read from the coin.  The low-bits test needs the canonical value: one Montgomery reduction of
// element 0 per lane, next to the permutation's 214 products.
static __global__ void __launch_bounds__(NT) hades_coin_pow_grind(const State* __restrict__ coin, unsigned long long base, unsigned long long count, unsigned bits,
                                                                  unsigned long long* found) {
    const unsigned long long i = (unsigned long long)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    const unsigned long long nonce = base + i;
    E s0 = mspos::load_e(coin->digest), s1 = small(nonce), s2 = tag_pow();
    mspos::permute(s0, s1, s2);
    const uint64_t t0 = f252::from_mont(s0).l[0];
    if ((t0 & ((1ull << bits) - 1)) == 0) atomicMin(found, nonce);            // bits <= 63
}

}  // namespace mshades
