// The RPO-256 public coin: an algebraic Fiat-Shamir transcript with its state resident on the device (ms_rpo_coin_* of
// include/ministark_hip_rpo_coin.h).  The coin is a 12-element sponge over Goldilocks on msrpo::permute (rpo_kernels.h): capacity
// s[0..4), rate s[4..12).  It absorbs field elements directly (no per-element digest), draws field elements without a rejection loop,
// and keeps no seed, counter or unread bytes -- which is why it is not a fifth instance of mscoin::coin_step.
//
// State (ms_rpo_coin_state, 128 bytes in HBM): s[12] in Montgomery form, pos in 4..12 = the next unread rate element (12: nothing
// unread), seven zero pad words.  The rules (the project's own, modelled on Miden's RpoRandomCoin):
//   create          s = 0; s[4..8) = seed; permute; pos = 4                      (the host writes the record, the kernel permutes)
//   reseed_digest   s[4+i] += d[i], i < 4; permute; pos = 4
//   reseed_int      s[4] += v mod 2^32; s[5] += v >> 32; permute; pos = 4
//   reseed_elements the base-field words in memory order, then a single 1, then zeros up to a multiple of 8; per block of 8:
//                   s[4+j] += w[j], permute; finally pos = 4
//   draw            per base-field word: if pos == 12 { permute; pos = 4 }; output s[pos++]
//   queries         (draw as a canonical integer) & (domain_size - 1)
//   grind           nonce n is accepted when permute(s with s[4] += n mod 2^32, s[5] += n >> 32)[0], as a canonical integer, has its
//                   low `bits` bits zero: a CAPACITY element, so that the state after reseed_int(n) hides the condition from every draw
// The chain is a sequence of dependent permutations, latency-bound.  One lane walking msrpo::permute takes a whole permutation's
// dependent length times twelve elements; here (Wide) state element j lives in lane j of ONE wave, each lane runs its own S-box chains and
// the two MDS products of a round gather the twelve elements through LDS (msrpo::mds_wide).  The integer arithmetic per element is that of
// msrpo::permute, so the words are the same.  Consecutive permutations of a call (the blocks of reseed_elements, the refills of a long
// draw) stay in registers: the record is loaded once and stored once per launch.  Narrow is the one-lane form of the same kernel, kept
// for the measurement of scripts/rpo_coin_probe.py; the library launches Wide.  Only the proof-of-work search is a wide launch.
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "gl_dev.h"
#include "rpo_kernels.h"

namespace msrpocoin {

static constexpr int WAVE = 64;
static constexpr int NT = 256;                  // the proof-of-work search

// the device image of ms_rpo_coin_state
struct State {
    uint64_t s[12];
    uint32_t pos;
    uint32_t pad[7];
};
static_assert(sizeof(State) == 128, "ms_rpo_coin_state is 128 bytes");

// State element j in lane j < 12; lanes 12..63 shadow element (lane mod 12) so that every lane reaches every barrier (results unused).
struct Wide {
    uint64_t s;
    uint64_t* sh;
    uint32_t row[12];
    unsigned j;
    bool owner;
    __device__ __forceinline__ void load(const State* coin, uint64_t* lds) {
        owner = threadIdx.x < 12;
        j = threadIdx.x % 12;
        sh = lds;
        #pragma unroll
        for (int n = 0; n < 12; n++) row[n] = msrpo::MDS_ROW[(n + 12 - j) % 12];
        s = coin->s[j];
    }
    __device__ __forceinline__ void store(State* coin, unsigned pos) const {
        if (owner) coin->s[j] = s;
        if (threadIdx.x == 0) coin->pos = pos;
    }
    // s[4 + q] += word(q) for q < 8
    template <class F> __device__ __forceinline__ void absorb(F word) {
        if (j >= 4) s = gl::add(s, word(j - 4));
    }
    __device__ __forceinline__ void permute() {
        for (int r = 0; r < 7; r++) {
            s = msrpo::mds_wide(s, sh, j, owner, row);
            s = msrpo::pow7(gl::add(s, msrpo::RC0[r * 12 + j]));
            s = msrpo::mds_wide(s, sh, j, owner, row);
            s = msrpo::pow_inv7(gl::add(s, msrpo::RC1[r * 12 + j]));
        }
    }
    // take(k, s[first + k]) for k < n; first + n <= 12
    template <class F> __device__ __forceinline__ void emit(unsigned first, unsigned n, F take) const {
        if (owner && j >= first && j < first + n) take(j - first, s);
    }
};

// The whole state in every lane's registers, msrpo::permute as the commitments run it; lane 0 stores.
struct Narrow {
    msrpo::State st;
    __device__ __forceinline__ void load(const State* coin, uint64_t*) {
        #pragma unroll
        for (int n = 0; n < 12; n++) st.s[n] = coin->s[n];
    }
    __device__ __forceinline__ void store(State* coin, unsigned pos) const {
        if (threadIdx.x != 0) return;
        #pragma unroll
        for (int n = 0; n < 12; n++) coin->s[n] = st.s[n];
        coin->pos = pos;
    }
    template <class F> __device__ __forceinline__ void absorb(F word) {
        #pragma unroll
        for (int q = 0; q < 8; q++) st.s[4 + q] = gl::add(st.s[4 + q], word((unsigned)q));
    }
    __device__ __forceinline__ void permute() { msrpo::permute(st); }
    template <class F> __device__ __forceinline__ void emit(unsigned first, unsigned n, F take) const {
        if (threadIdx.x != 0) return;
        #pragma unroll
        for (int q = 4; q < 12; q++)
            if ((unsigned)q >= first && (unsigned)q < first + n) take((unsigned)q - first, st.s[q]);
    }
};

enum { OP_CREATE = 0, OP_RESEED_DIGEST = 1, OP_RESEED_INT = 2, OP_RESEED_ELEMENTS = 3, OP_DRAW = 4, OP_QUERIES = 5 };

// One step of the chain.  `in`: the four words of a digest, or `count` >= 1 base-field words of elements; `arg`: the integer of
// reseed_int, or domain_size - 1 for the query samples; `out`: `count` base-field words (an Fq3 element is three of them) or samples.
template <class SP, int OP>
static __global__ void __launch_bounds__(WAVE) rpo_coin_step(State* coin, const uint64_t* __restrict__ in, uint64_t arg, size_t count, uint64_t* __restrict__ out) {
    __shared__ uint64_t sh[12];
    SP sp;
    sp.load(coin, sh);
    unsigned pos = coin->pos;
    __syncthreads();                                     // every lane has read the record before any lane stores to it
    if constexpr (OP == OP_CREATE) {
        sp.permute();
        pos = 4;
    } else if constexpr (OP == OP_RESEED_DIGEST) {
        sp.absorb([&](unsigned q) { return q < 4 ? in[q] : 0ull; });
        sp.permute();
        pos = 4;
    } else if constexpr (OP == OP_RESEED_INT) {
        const uint64_t lo = gld::mmul(arg & 0xFFFFFFFFull, gl::R2), hi = gld::mmul(arg >> 32, gl::R2);     // both halves < 2^32 < p
        sp.absorb([&](unsigned q) { return q == 0 ? lo : q == 1 ? hi : 0ull; });
        sp.permute();
        pos = 4;
    } else if constexpr (OP == OP_RESEED_ELEMENTS) {
        for (size_t base = 0; base <= count; base += 8) {                    // count / 8 + 1 blocks: the 1 always has a place
            sp.absorb([&](unsigned q) {
                const size_t idx = base + q;
                return idx < count ? in[idx] : idx == count ? gl::ONE_MONT : 0ull;
            });
            sp.permute();
        }
        pos = 4;
    } else {
        for (size_t i = 0; i < count;) {
            if (pos == 12) { sp.permute(); pos = 4; }
            const unsigned n = (unsigned)(count - i < (size_t)(12 - pos) ? count - i : (size_t)(12 - pos));
            sp.emit(pos, n, [&](unsigned k, uint64_t v) {
                if constexpr (OP == OP_QUERIES) out[i + k] = gld::mmul(v, 1) & arg;
                else out[i + k] = v;
            });
            i += n;
            pos += n;
        }
    }
    sp.store(coin, pos);
}

// One nonce per lane, the full-width permutation per lane as in rpo256_merge_level; the state is read from the coin.
static __global__ void __launch_bounds__(NT) rpo_coin_pow_grind(const State* __restrict__ coin, unsigned long long base, unsigned long long count, unsigned bits,
                                                                unsigned long long* found) {
    const unsigned long long i = (unsigned long long)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    const unsigned long long nonce = base + i;
    msrpo::State st;
    #pragma unroll
    for (int n = 0; n < 12; n++) st.s[n] = coin->s[n];
    st.s[4] = gl::add(st.s[4], gld::mmul(nonce & 0xFFFFFFFFull, gl::R2));
    st.s[5] = gl::add(st.s[5], gld::mmul(nonce >> 32, gl::R2));
    msrpo::permute(st);
    const uint64_t t0 = gld::mmul(st.s[0], 1);
    if ((t0 & ((1ull << bits) - 1)) == 0) atomicMin(found, nonce);          // bits <= 63
}

}  // namespace msrpocoin
