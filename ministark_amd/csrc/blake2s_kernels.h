// BLAKE2s-256 Merkle commitments and proof-of-work for gfx950: the fast choice of H in MatrixMerkleTreeImpl<H>
// (src/merkle.rs:296-361) and PublicCoinImpl<F, H> (src/random.rs:61-141), through the reference's HashFn / ElementHashFn
// seam (src/hash.rs:9-41).  H = unkeyed BLAKE2s with a 32-byte digest (RFC 7693; blake2::Blake2s256, hashlib.blake2s).
//   leaf[r]   = H( ||_c canonical little-endian bytes of M[c][r] )   -- the bytes ms_sha256_rows feeds SHA-256
//               (Fp: 8 bytes, Fq3: c0||c1||c2, Fp252: 32 bytes); a row of L bytes is max(1, ceil(L / 64)) blocks, the last one
//               zero-padded, with counter t = L and the final flag (L = 0: one zero block, t = 0)
//   nodes[k]  = H(nodes[2k] || nodes[2k+1]): ONE 64-byte block (SHA-256 needs two compressions: the data and the padding)
//   pow       = H(seed32 || nonce as 8 big-endian bytes): one 40-byte block
// BLAKE2s is little-endian throughout, so canonical limbs and digests go in and out of the state without byte swaps.
// Layout and launch shapes are those of sha256_kernels.h: one row (or node) per lane, column reads coalesced, the top of a tree
// climbed in LDS by one workgroup per subtree.  A compression is 10 rounds x 8 G = 80 x (2 v_add3_u32 + 2 v_add_u32 + 4 v_xor_b32
// + 4 rotations, one v_alignbit_b32 / v_perm_b32 each); the message permutation SIGMA is resolved at compile time (fully unrolled
// rounds: m[SIGMA[r][i]] is a register name, not a load).
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "gl_dev.h"
#include "fp252.h"

namespace msb2s {

static constexpr int MAXCOLS = 128;
static constexpr int NT = 256;

static constexpr uint32_t IV0 = 0x6A09E667u, IV1 = 0xBB67AE85u, IV2 = 0x3C6EF372u, IV3 = 0xA54FF53Au;
static constexpr uint32_t IV4 = 0x510E527Fu, IV5 = 0x9B05688Cu, IV6 = 0x1F83D9ABu, IV7 = 0x5BE0CD19u;
// parameter block word 0 of an unkeyed 32-byte digest: digest length 32, key length 0, fanout 1, depth 1
static constexpr uint32_t PARAM0 = 0x01010020u;

static constexpr uint8_t SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }   // -> v_alignbit_b32 / v_perm_b32
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
#else
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
#endif

__device__ __forceinline__ void G(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t x, uint32_t y) {
    a = a + b + x; d = rotr(d ^ a, 16);                   // a + b + x -> v_add3_u32
    c = c + d;     b = rotr(b ^ c, 12);
    a = a + b + y; d = rotr(d ^ a, 8);
    c = c + d;     b = rotr(b ^ c, 7);
}

struct B2s {
    uint32_t h[8];
    uint32_t m[16];
    __device__ __forceinline__ void init() {
        h[0] = IV0 ^ PARAM0; h[1] = IV1; h[2] = IV2; h[3] = IV3; h[4] = IV4; h[5] = IV5; h[6] = IV6; h[7] = IV7;
    }
    // one compression of the 16 little-endian words in m[]: t = bytes hashed so far (< 2^32 here), last = final block
    __device__ __forceinline__ void compress(uint32_t t, bool last) {
        uint32_t v[16] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7],
                          IV0, IV1, IV2, IV3, IV4 ^ t, IV5, last ? ~IV6 : IV6, IV7};
        #pragma unroll
        for (int r = 0; r < 10; r++) {
            G(v[0], v[4], v[8], v[12], m[SIGMA[r][0]], m[SIGMA[r][1]]);
            G(v[1], v[5], v[9], v[13], m[SIGMA[r][2]], m[SIGMA[r][3]]);
            G(v[2], v[6], v[10], v[14], m[SIGMA[r][4]], m[SIGMA[r][5]]);
            G(v[3], v[7], v[11], v[15], m[SIGMA[r][6]], m[SIGMA[r][7]]);
            G(v[0], v[5], v[10], v[15], m[SIGMA[r][8]], m[SIGMA[r][9]]);
            G(v[1], v[6], v[11], v[12], m[SIGMA[r][10]], m[SIGMA[r][11]]);
            G(v[2], v[7], v[8], v[13], m[SIGMA[r][12]], m[SIGMA[r][13]]);
            G(v[3], v[4], v[9], v[14], m[SIGMA[r][14]], m[SIGMA[r][15]]);
        }
        #pragma unroll
        for (int i = 0; i < 8; i++) h[i] = xor3(h[i], v[i], v[i + 8]);
    }
    // H(64 bytes at p): the Merkle merge, one final block of 64 bytes
    __device__ __forceinline__ void merge(const uint4* __restrict__ p) {
        #pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 x = p[q];
            m[4 * q] = x.x; m[4 * q + 1] = x.y; m[4 * q + 2] = x.z; m[4 * q + 3] = x.w;
        }
        init();
        compress(64, true);
    }
    __device__ __forceinline__ void put(uint8_t* out) const {
        uint4* o = (uint4*)out;
        o[0] = make_uint4(h[0], h[1], h[2], h[3]);
        o[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
};

struct RowsParams {
    const uint64_t* cols[MAXCOLS];
    uint8_t* leaves;          // nrows x 32 bytes
    size_t nrows;
    unsigned ncols;
    unsigned row_stride;      // words between consecutive rows of one column (V when columns are dense)
};

// One row per lane; V = u64 words per element (1 Fp, 3 Fq3, 4 Fp252).  The message is a stream of 8-byte slots: slot i < nslots is
// limb (i % V) of the element of column i / V as its canonical value, two little-endian words.  A block is 8 slots, filled with
// compile-time register indices; slots past the end are zero.
template <int V>
static __global__ void __launch_bounds__(NT) blake2s_rows(RowsParams P) {
    const size_t r = (size_t)blockIdx.x * NT + threadIdx.x;
    if (r >= P.nrows) return;
    B2s s;
    s.init();
    const unsigned nslots = P.ncols * V;
    const unsigned nblocks = nslots ? (nslots + 7) / 8 : 1;
    f252::E big = f252::zero();
    for (unsigned blk = 0; blk < nblocks; blk++) {
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned i = blk * 8 + j;
            uint64_t x = 0;
            if (i < nslots) {
                const unsigned c = i / V, v = i - c * V;
                const uint64_t* __restrict__ e = P.cols[c] + r * P.row_stride;
                if constexpr (V == 4) {                                  // 4 | 8: the limb is j % 4, known here
                    if ((j & 3) == 0) big = f252::from_mont(f252::E{{e[0], e[1], e[2], e[3]}});
                    x = big.l[j & 3];
                } else {
                    x = gld::mmul(e[v], 1);                              // out of Montgomery form, canonical
                }
            }
            s.m[2 * j] = (uint32_t)x; s.m[2 * j + 1] = (uint32_t)(x >> 32);
        }
        const bool last = blk + 1 == nblocks;
        s.compress(last ? nslots * 8 : (blk + 1) * 64, last);
    }
    s.put(P.leaves + r * 32);
}

// nodes[out0 + i] = H(src[2i] || src[2i+1]) for i < count; digests are 32 raw bytes
static __global__ void __launch_bounds__(NT) blake2s_merge_level(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t count) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    B2s s;
    s.merge((const uint4*)(src + i * 64));
    s.put(dst + i * 32);
}

// The upper levels of a tree in few launches, as sha256_merkle_top: workgroup b takes the NT parents [b NT, b NT + NT) of a level of
// `count` parents (count = NT: the top of the tree; count = k NT: k subtrees at once; count < NT: the tree's last levels), keeps the
// current level in LDS and climbs to ONE node, writing every level to its slot of nodes[].  PER = 2: a lane computes two adjacent
// parents and their parent in registers (half the workgroups for the widest of these levels).
template <int PER>
static __global__ void __launch_bounds__(NT) blake2s_merkle_top(const uint8_t* __restrict__ src, uint8_t* __restrict__ nodes, unsigned count) {
    __shared__ uint32_t lvl[2][NT * 8];
    const unsigned t = threadIdx.x, b = blockIdx.x;
    if (count <= (unsigned)NT && b == 0 && t < 8) ((uint32_t*)nodes)[t] = 0;     // the launch that ends in the root clears nodes[0]
    unsigned mine = count < (unsigned)NT ? count : (unsigned)NT;
    size_t level = count;
    B2s s;
    if constexpr (PER == 2) {                                            // count is a multiple of 2 NT here
        const size_t n0 = (size_t)b * 2 * NT + 2 * t;
        uint4 second[4];                                                  // both messages are requested before the first compression
        const uint4* in2 = (const uint4*)(src + (n0 + 1) * 64);
        #pragma unroll
        for (int q = 0; q < 4; q++) second[q] = in2[q];
        s.merge((const uint4*)(src + n0 * 64));
        s.put(nodes + (level + n0) * 32);
        uint32_t left[8];
        #pragma unroll
        for (int q = 0; q < 8; q++) left[q] = s.h[q];
        s.merge(second);
        s.put(nodes + (level + n0 + 1) * 32);
        #pragma unroll
        for (int q = 0; q < 8; q++) { s.m[8 + q] = s.h[q]; s.m[q] = left[q]; }
        level >>= 1;
        s.init();
        s.compress(64, true);
    } else if (t < mine) {
        s.merge((const uint4*)(src + ((size_t)b * NT + t) * 64));
    }
    int cur = 0;
    for (;;) {
        if (t < mine) {
            s.put(nodes + (level + (size_t)b * mine + t) * 32);
            #pragma unroll
            for (int q = 0; q < 8; q++) lvl[cur][t * 8 + q] = s.h[q];
        }
        if (mine == 1) break;
        __syncthreads();
        mine >>= 1; level >>= 1;
        if (t < mine) {
            #pragma unroll
            for (int q = 0; q < 16; q++) s.m[q] = lvl[cur][t * 16 + q];
            s.init();
            s.compress(64, true);
        }
        cur ^= 1;
    }
}

// Proof-of-work (PublicCoin::grind_proof_of_work, src/random.rs:48-55, 129-132, 180-192): the smallest nonce >= 1 with
// leading_zeros(H(seed || nonce.to_be_bytes())) >= bits.  One nonce per lane over [base, base + count); the minimum hit is kept with
// atomicMin.  seed[] holds the 32 seed bytes as little-endian words (wave-uniform).
struct PowParams { uint32_t seed[8]; unsigned long long base; unsigned long long count; unsigned bits; unsigned long long* found; };
static __global__ void __launch_bounds__(NT) blake2s_pow_grind(PowParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * NT + threadIdx.x;
    if (i >= P.count) return;
    const unsigned long long nonce = P.base + i;
    B2s s;
    s.init();
    #pragma unroll
    for (int q = 0; q < 8; q++) s.m[q] = P.seed[q];
    s.m[8] = __builtin_bswap32((uint32_t)(nonce >> 32)); s.m[9] = __builtin_bswap32((uint32_t)nonce);   // big-endian u64 bytes
    #pragma unroll
    for (int q = 10; q < 16; q++) s.m[q] = 0;
    s.compress(40, true);
    // mshash::leading_zero_bits<false>(s.h), written out: through the function this kernel's register and instruction counts move
    // (profiles/r10_kernel_resources*.txt)
    unsigned lz = 0;
    bool done = false;
    #pragma unroll
    for (int q = 0; q < 8; q++) {
        if (!done) {
            const uint32_t w = __builtin_bswap32(s.h[q]);
            const unsigned z = w ? (unsigned)__clz(w) : 32u;
            lz += z;
            if (z != 32) done = true;
        }
    }
    if (lz >= P.bits) atomicMin(P.found, nonce);
}

}  // namespace msb2s
