// The public coin of the Fiat-Shamir transcript, resident on the device: PublicCoinImpl<F, H> (src/random.rs:61-141) as
// ProverChannel drives it (src/channel.rs:46-100, src/fri.rs:217-247), for H = SHA-256, BLAKE2s-256, Keccak-256, SHA3-256 and BLAKE3
// (the template parameter H is ms_coin_create's hash id: 0, 1, 3, 4, 6; 5 stays unknown, and so does 2 -- the RPO-256 coin is a sponge, not a seed and a counter, and has a family of its own: rpo_coin_kernels.h, ms_rpo_coin_*).
//
// State (ms_coin_state of include/ministark_hip_transcript.h, 80 bytes in HBM): a 32-byte seed, a u64 counter and up to 32 unread bytes of the
// last digest.  The rules, one device function each:
//   refill          counter += 1; unread = H(seed || counter as 8 big-endian bytes)
//   next_word       8 unread bytes popped from the END, most significant first: the words of a digest D come out as
//                   LE64(D[24..32]), LE64(D[16..24]), LE64(D[8..16]), LE64(D[0..8]); every consumer takes whole words
//   reseed          seed = H(seed || digest32), counter = 0, nothing unread        (HashFn::merge)
//   reseed_int      seed = H(seed || v as 8 big-endian bytes), counter = 0, nothing unread   (HashFn::merge_with_int)
//   element_digest  H(canonical little-endian bytes of one element): the bytes ms_sha256_rows hashes for a one-column row
//   draw            ark-ff 0.4.2's Standard sampler: N words as limbs 0..N-1, the top 64 N - bits(p) bits of the last limb cleared,
//                   all N words discarded when the integer is >= p; the accepted limbs ARE the Montgomery representation
//   sample_below    rand 0.8.5's gen_range(0..range) for u64: zone = (range << clz(range)) - 1; take words v until the low half of
//                   v * range is <= zone, the high half is the sample
// These are dependent chains of a few compressions: latency-bound, no roofline.  Every kernel is ONE wave; lane 0 walks the chain
// (the state lives in its registers between the load and the store), and in coin_reseed_elements all 64 lanes hash the per-element
// digests of a batch in parallel before lane 0 merges them in order.  The compression functions are those of sha256_kernels.h /
// blake2s_kernels.h / keccak_sponge.h / blake3_kernels.h (every message here is one Keccak block and one BLAKE3 block; the chains keep the permutation as a short loop).  Only the proof-of-work search (one nonce per lane, as sha256_pow_grind) is a wide launch.
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "gl_dev.h"
#include "fp252.h"
#include "sha256_kernels.h"
#include "blake2s_kernels.h"
#include "keccak_sponge.h"
#include "blake3_kernels.h"

namespace mscoin {

static constexpr int WAVE = 64;
static constexpr int NT = 256;                  // the proof-of-work search

// the device image of ms_coin_state; digests and seeds are kept as the little-endian words of their bytes
struct State {
    uint32_t seed[8];
    uint64_t counter;
    uint32_t nbytes, pad;
    uint32_t unread[8];                          // bytes [0, nbytes) are unread; consumed bytes are cleared
};
static_assert(sizeof(State) == 80, "ms_coin_state is 80 bytes");

// H(the first `len` bytes of m): m[] holds the message as little-endian words, zero past its end; len is 8, 24, 32, 40 or 64.
// out[] = the digest's bytes as little-endian words.
template <int H>
__device__ __forceinline__ void hash_short(const uint32_t (&m)[16], unsigned len, uint32_t (&out)[8]) {
    if constexpr (H == 0) {                      // SHA-256: big-endian words, 0x80, zeros, the bit length in the last word
        mssha::Sha s;
        s.init();
        #pragma unroll
        for (int q = 0; q < 16; q++) s.w[q] = mssha::bswap32(m[q]);
        if (len < 64) {
            #pragma unroll
            for (int q = 2; q < 15; q++) if ((unsigned)q == len / 4) s.w[q] = 0x80000000u;
            s.w[15] = len * 8;
            s.compress();
        } else {
            s.compress();
            s.compress_kw(mssha::KW_PAD64);
        }
        #pragma unroll
        for (int q = 0; q < 8; q++) out[q] = mssha::bswap32(s.h[q]);
    } else if constexpr (H == 3 || H == 4) {     // Keccak-256 / SHA3-256: one block, the domain byte at offset len, 0x80 in byte 135
        mskec::Keccak s;
        s.load_short(m, len / 8, H == 3 ? mskec::DOMAIN_KECCAK : mskec::DOMAIN_SHA3);
        s.permute<mskec::UNROLL_CHAIN>();
        s.digest(out);
    } else if constexpr (H == 6) {               // BLAKE3: one block that is the whole input, block_len = len
        msb3::B3 s;
        s.init();
        #pragma unroll
        for (int q = 0; q < 16; q++) s.m[q] = m[q];
        s.compress(0, len, msb3::ONE_BLOCK);
        #pragma unroll
        for (int q = 0; q < 8; q++) out[q] = s.cv[q];
    } else {                                     // BLAKE2s: one final block, counter = len
        static_assert(H == 1, "hash ids: 0 SHA-256, 1 BLAKE2s-256, 3 Keccak-256, 4 SHA3-256, 6 BLAKE3");
        msb2s::B2s s;
        s.init();
        #pragma unroll
        for (int q = 0; q < 16; q++) s.m[q] = m[q];
        s.compress(len, true);
        #pragma unroll
        for (int q = 0; q < 8; q++) out[q] = s.h[q];
    }
}

// H(a || v as 8 big-endian bytes): merge_with_int (src/hash.rs:84-89)
template <int H>
__device__ __forceinline__ void merge_with_int(const uint32_t (&a)[8], uint64_t v, uint32_t (&out)[8]) {
    uint32_t m[16];
    #pragma unroll
    for (int q = 0; q < 8; q++) m[q] = a[q];
    m[8] = __builtin_bswap32((uint32_t)(v >> 32)); m[9] = __builtin_bswap32((uint32_t)v);
    #pragma unroll
    for (int q = 10; q < 16; q++) m[q] = 0;
    hash_short<H>(m, 40, out);
}

template <int H>
__device__ __forceinline__ void refill(State& S) {
    S.counter += 1;
    merge_with_int<H>(S.seed, S.counter, S.unread);
    S.nbytes = 32;
}

template <int H>
__device__ __forceinline__ uint64_t next_word(State& S) {
    if (S.nbytes == 0) refill<H>(S);
    uint64_t w = 0;
    #pragma unroll
    for (int q = 0; q < 4; q++)                   // the last 8 unread bytes, i.e. words nbytes / 4 - 2 and nbytes / 4 - 1
        if ((unsigned)(2 * q + 2) == S.nbytes / 4) { w = S.unread[2 * q] | ((uint64_t)S.unread[2 * q + 1] << 32); S.unread[2 * q] = 0; S.unread[2 * q + 1] = 0; }
    S.nbytes -= 8;
    return w;
}

__device__ __forceinline__ void clear_unread(State& S) {
    S.counter = 0; S.nbytes = 0;
    #pragma unroll
    for (int q = 0; q < 8; q++) S.unread[q] = 0;
}

template <int H>
__device__ __forceinline__ void reseed(State& S, const uint32_t (&d)[8]) {
    uint32_t m[16];
    #pragma unroll
    for (int q = 0; q < 8; q++) { m[q] = S.seed[q]; m[8 + q] = d[q]; }
    hash_short<H>(m, 64, S.seed);
    clear_unread(S);
}

template <int H>
__device__ __forceinline__ void reseed_int(State& S, uint64_t v) {
    uint32_t next[8];
    merge_with_int<H>(S.seed, v, next);
    #pragma unroll
    for (int q = 0; q < 8; q++) S.seed[q] = next[q];
    clear_unread(S);
}

// H(bytes(e)) for element e of a column of V-word elements in Montgomery form (V = 1 Fp, 3 Fq3, 4 Fp252)
template <int H, int V>
__device__ __forceinline__ void element_digest(const uint64_t* __restrict__ e, uint32_t (&out)[8]) {
    uint64_t c[4] = {0, 0, 0, 0};
    if constexpr (V == 4) {
        const f252::E x = f252::from_mont(f252::E{{e[0], e[1], e[2], e[3]}});
        c[0] = x.l[0]; c[1] = x.l[1]; c[2] = x.l[2]; c[3] = x.l[3];
    } else {
        #pragma unroll
        for (int v = 0; v < V; v++) c[v] = gld::mmul(e[v], 1);
    }
    uint32_t m[16];
    #pragma unroll
    for (int q = 0; q < 4; q++) { m[2 * q] = (uint32_t)c[q]; m[2 * q + 1] = (uint32_t)(c[q] >> 32); }
    #pragma unroll
    for (int q = 8; q < 16; q++) m[q] = 0;
    hash_short<H>(m, 8 * V, out);
}

// one base-field element into out[0 .. N): N = 1 Goldilocks, N = 4 Fp252
template <int H, int N>
__device__ __forceinline__ void draw_base(State& S, uint64_t* out) {
    for (;;) {
        if constexpr (N == 1) {
            const uint64_t w = next_word<H>(S);                       // 64 - bits(p) = 0 bits to clear
            if (w < gl::P) { out[0] = w; return; }
        } else {
            f252::E x;
            #pragma unroll
            for (int q = 0; q < 4; q++) x.l[q] = next_word<H>(S);
            x.l[3] &= (~0ull) >> 4;                                   // 256 - 252 bits
            if (!f252::geq_p(x)) { out[0] = x.l[0]; out[1] = x.l[1]; out[2] = x.l[2]; out[3] = x.l[3]; return; }
        }
    }
}

template <int H>
__device__ __forceinline__ uint64_t sample_below(State& S, uint64_t range) {
    const uint64_t zone = (range << __builtin_clzll(range)) - 1;
    for (;;) {
        const gl::u128 prod = (gl::u128)next_word<H>(S) * range;
        if ((uint64_t)prod <= zone) return (uint64_t)(prod >> 64);
    }
}

__device__ __forceinline__ void load_digest(const uint32_t* __restrict__ p, uint32_t (&d)[8]) {
    #pragma unroll
    for (int q = 0; q < 8; q++) d[q] = p[q];
}

enum { OP_RESEED_DIGEST = 0, OP_RESEED_INT = 1, OP_DRAW_FP = 2, OP_DRAW_FP252 = 3, OP_QUERIES = 4 };

// One step of the chain on lane 0.  `count` words (OP_DRAW_FP: base-field elements, so 3 per Fq3 element), Fp252 elements or
// samples go to `out`; `arg` is the integer of reseed_int or the range of the query samples; `digest` the 32 bytes to absorb.
template <int H, int OP>
static __global__ void __launch_bounds__(WAVE) coin_step(State* coin, const uint32_t* __restrict__ digest, uint64_t arg, size_t count, uint64_t* __restrict__ out) {
    if (threadIdx.x != 0) return;
    State S = *coin;
    if constexpr (OP == OP_RESEED_DIGEST) {
        uint32_t d[8];
        load_digest(digest, d);
        reseed<H>(S, d);
    } else if constexpr (OP == OP_RESEED_INT) {
        reseed_int<H>(S, arg);
    } else if constexpr (OP == OP_DRAW_FP) {
        for (size_t i = 0; i < count; i++) draw_base<H, 1>(S, out + i);
    } else if constexpr (OP == OP_DRAW_FP252) {
        for (size_t i = 0; i < count; i++) draw_base<H, 4>(S, out + 4 * i);
    } else {
        for (size_t i = 0; i < count; i++) out[i] = sample_below<H>(S, arg);
    }
    *coin = S;
}

// reseed_with_field_elements (src/random.rs:70-75): for each e in order seed = H(seed || H(bytes(e))).  The lanes hash a batch of 64
// element digests into LDS, lane 0 merges them in order; count >= 1.
template <int H, int V>
static __global__ void __launch_bounds__(WAVE) coin_reseed_elements(State* coin, const uint64_t* __restrict__ elems, size_t count) {
    __shared__ uint32_t dig[WAVE][8];
    const unsigned t = threadIdx.x;
    State S;
    if (t == 0) S = *coin;
    for (size_t base = 0; base < count; base += WAVE) {
        if (base + t < count) {
            uint32_t d[8];
            element_digest<H, V>(elems + (base + t) * V, d);
            #pragma unroll
            for (int q = 0; q < 8; q++) dig[t][q] = d[q];
        }
        __syncthreads();
        if (t == 0) {
            const unsigned n = (unsigned)(count - base < (size_t)WAVE ? count - base : (size_t)WAVE);
            for (unsigned k = 0; k < n; k++) {
                uint32_t d[8];
                #pragma unroll
                for (int q = 0; q < 8; q++) d[q] = dig[k][q];
                reseed<H>(S, d);
            }
        }
        __syncthreads();
    }
    if (t == 0) *coin = S;
}

// grind_proof_of_work (src/random.rs:48-55) with the seed read from the coin's state: the launch shape of sha256_pow_grind
template <int H>
static __global__ void __launch_bounds__(NT) coin_pow_grind(const State* __restrict__ coin, unsigned long long base, unsigned long long count, unsigned bits,
                                                            unsigned long long* found) {
    const unsigned long long i = (unsigned long long)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    const unsigned long long nonce = base + i;
    uint32_t seed[8], d[8];
    load_digest(coin->seed, seed);
    merge_with_int<H>(seed, nonce, d);
    // mshash::leading_zero_bits<false>(d), written out: through the function these kernels' instruction counts move
    // (profiles/r10_kernel_resources*.txt)
    unsigned lz = 0;
    bool done = false;
    #pragma unroll
    for (int q = 0; q < 8; q++) {
        if (!done) {
            const uint32_t w = __builtin_bswap32(d[q]);
            const unsigned z = w ? (unsigned)__clz(w) : 32u;
            lz += z;
            if (z != 32) done = true;
        }
    }
    if (lz >= bits) atomicMin(found, nonce);
}

}  // namespace mscoin
