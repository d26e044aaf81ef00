// BLAKE3 Merkle commitments and proof-of-work for gfx950: the byte hash STARK provers outside this project default to, as a choice of
// H in MatrixMerkleTreeImpl<H> (src/merkle.rs:296-361) and PublicCoinImpl<F, H> (src/random.rs:61-141), through the reference's
// HashFn / ElementHashFn seam (src/hash.rs:9-41).  H = unkeyed BLAKE3 in its default hash mode with a 32-byte digest.
//   leaf[r]   = H( ||_c canonical little-endian bytes of M[c][r] )   -- the bytes ms_sha256_rows / ms_blake2s_rows hash
//   nodes[k]  = H(nodes[2k] || nodes[2k+1]): the plain hash of 64 bytes, ONE compression (flags CHUNK_START | CHUNK_END | ROOT,
//               counter 0, block_len 64) -- not BLAKE3's parent-node mode
//   pow       = H(seed32 || nonce as 8 big-endian bytes): one block, block_len 40
// The compression is BLAKE2s's G (blake2s_kernels.h) on the same sixteen words with 7 rounds instead of 10:
//   v = cv[0..8] || IV[0..4] || counter_lo, counter_hi, block_len, flags;  7 x (four column G, four diagonal G);  cv' = v[i] ^ v[i + 8]
// with the message words permuted between rounds by m'[i] = m[PERM[i]] -- resolved at compile time (MSG[r][i], fully unrolled rounds:
// m[MSG[r][i]] is a register name, as SIGMA is in BLAKE2s).  What BLAKE3 is not BLAKE2s: input longer than 1024 bytes is a tree.
//   chunks   1024 bytes each (the empty input is one empty chunk), 64-byte blocks, the last one zero-padded with block_len = its real
//            bytes; every block of chunk c has counter = c, the first carries CHUNK_START, the last CHUNK_END
//   parents  compress(IV, left_cv || right_cv, 0, 64, PARENT); the left subtree takes the largest power of two of chunks that is
//            smaller than the chunk count
//   ROOT     on the last compression only: the last block of a single chunk, or the top parent
// A row is at most 128 columns x 32 bytes = 4 chunks, so the shapes are p(c0, c1), p(p(c0, c1), c2) and p(p(c0, c1), p(c2, c3)).
// Layout and launch shapes are those of sha256_kernels.h / blake2s_kernels.h: one row (or node) per lane, column reads coalesced, the
// top of a tree climbed in LDS by one workgroup per subtree.  BLAKE3 is little-endian throughout: no byte swaps.
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "gl_dev.h"
#include "fp252.h"
#include "blake2s_kernels.h"

namespace msb3 {

using msb2s::G;
using msb2s::IV0; using msb2s::IV1; using msb2s::IV2; using msb2s::IV3;
using msb2s::IV4; using msb2s::IV5; using msb2s::IV6; using msb2s::IV7;

static constexpr int MAXCOLS = msb2s::MAXCOLS;
static constexpr int NT = msb2s::NT;

static constexpr uint32_t CHUNK_START = 1, CHUNK_END = 2, PARENT = 4, ROOT = 8;
static constexpr uint32_t ONE_BLOCK = CHUNK_START | CHUNK_END | ROOT;          // a message of at most 64 bytes
static constexpr int CHUNK_BLOCKS = 16;                                       // 1024 bytes
static constexpr int MAXCHUNKS = MAXCOLS * 32 / 1024;

static constexpr uint8_t PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
// MSG[r][i]: the word of the block that round r takes as its i-th; MSG[r + 1][i] = MSG[r][PERM[i]]
static constexpr uint8_t MSG[7][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8},
    {3, 4, 10, 12, 13, 2, 7, 14, 6, 5, 9, 0, 11, 15, 8, 1}, {10, 7, 12, 9, 14, 3, 13, 15, 4, 0, 11, 2, 5, 8, 1, 6},
    {12, 13, 9, 11, 15, 10, 14, 8, 7, 2, 5, 3, 0, 1, 6, 4}, {9, 14, 11, 5, 8, 12, 15, 1, 13, 3, 0, 10, 2, 6, 4, 7},
    {11, 15, 5, 0, 1, 9, 8, 6, 14, 10, 2, 12, 3, 4, 7, 13}};
constexpr bool msg_follows_perm() {
    for (int r = 0; r + 1 < 7; r++)
        for (int i = 0; i < 16; i++)
            if (MSG[r + 1][i] != MSG[r][PERM[i]]) return false;
    return true;
}
static_assert(msg_follows_perm(), "MSG is PERM applied round after round");

struct B3 {
    uint32_t cv[8];
    uint32_t m[16];
    __device__ __forceinline__ void init() {
        cv[0] = IV0; cv[1] = IV1; cv[2] = IV2; cv[3] = IV3; cv[4] = IV4; cv[5] = IV5; cv[6] = IV6; cv[7] = IV7;
    }
    // one compression of the 16 little-endian words in m[]: counter = the chunk number (< 2^32 here), block_len = the block's real bytes
    __device__ __forceinline__ void compress(uint32_t counter, uint32_t block_len, uint32_t flags) {
        uint32_t v[16] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7],
                          IV0, IV1, IV2, IV3, counter, 0u, block_len, flags};
        #pragma unroll
        for (int r = 0; r < 7; r++) {
            G(v[0], v[4], v[8], v[12], m[MSG[r][0]], m[MSG[r][1]]);
            G(v[1], v[5], v[9], v[13], m[MSG[r][2]], m[MSG[r][3]]);
            G(v[2], v[6], v[10], v[14], m[MSG[r][4]], m[MSG[r][5]]);
            G(v[3], v[7], v[11], v[15], m[MSG[r][6]], m[MSG[r][7]]);
            G(v[0], v[5], v[10], v[15], m[MSG[r][8]], m[MSG[r][9]]);
            G(v[1], v[6], v[11], v[12], m[MSG[r][10]], m[MSG[r][11]]);
            G(v[2], v[7], v[8], v[13], m[MSG[r][12]], m[MSG[r][13]]);
            G(v[3], v[4], v[9], v[14], m[MSG[r][14]], m[MSG[r][15]]);
        }
        #pragma unroll
        for (int i = 0; i < 8; i++) cv[i] = v[i] ^ v[i + 8];
    }
    // H(64 bytes at p): the Merkle merge, one block that is a whole chunk and the root
    __device__ __forceinline__ void merge(const uint4* __restrict__ p) {
        #pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 x = p[q];
            m[4 * q] = x.x; m[4 * q + 1] = x.y; m[4 * q + 2] = x.z; m[4 * q + 3] = x.w;
        }
        init();
        compress(0, 64, ONE_BLOCK);
    }
    __device__ __forceinline__ void put(uint8_t* out) const {
        uint4* o = (uint4*)out;
        o[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
        o[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
    }
};

using RowsParams = msb2s::RowsParams;

// One row per lane; V = u64 words per element (1 Fp, 3 Fq3, 4 Fp252).  The message is blake2s_rows's stream of 8-byte slots: slot
// i < nslots is limb (i % V) of the element of column i / V as its canonical value; a block is 8 slots, a chunk 128.  The lane walks
// its chunks in order and keeps their chaining values in registers (c[k] is written under a wave-uniform compare, so k is a register
// name); the parents above them are one loop around one compression:
//   parent 0   (c0, c1) -> c0                                   the root of 2 chunks
//   parent 1   3 chunks: (c0, c2), the root;  4 chunks: (c2, c3) -> c2
//   parent 2   (c0, c2), the root of 4 chunks
template <int V>
static __global__ void __launch_bounds__(NT) blake3_rows(RowsParams P) {
    const size_t r = (size_t)blockIdx.x * NT + threadIdx.x;
    if (r >= P.nrows) return;
    B3 s;
    s.init();
    const unsigned nslots = P.ncols * V;
    const unsigned nblocks = nslots ? (nslots + 7) / 8 : 1;
    const unsigned nchunks = (nblocks + CHUNK_BLOCKS - 1) / CHUNK_BLOCKS;          // 1..4: ncols <= MAXCOLS is the host's check
    uint32_t c[MAXCHUNKS][8] = {};
    f252::E big = f252::zero();
    for (unsigned blk = 0; blk < nblocks; blk++) {
        const unsigned chunk = blk / CHUNK_BLOCKS, at = blk % CHUNK_BLOCKS;
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned i = blk * 8 + j;
            uint64_t x = 0;
            if (i < nslots) {
                const unsigned col = i / V, v = i - col * V;
                const uint64_t* __restrict__ e = P.cols[col] + r * P.row_stride;
                if constexpr (V == 4) {                                  // 4 | 8: the limb is j % 4, known here
                    if ((j & 3) == 0) big = f252::from_mont(f252::E{{e[0], e[1], e[2], e[3]}});
                    x = big.l[j & 3];
                } else {
                    x = gld::mmul(e[v], 1);                              // out of Montgomery form, canonical
                }
            }
            s.m[2 * j] = (uint32_t)x; s.m[2 * j + 1] = (uint32_t)(x >> 32);
        }
        const bool last = blk + 1 == nblocks, end = last || at == CHUNK_BLOCKS - 1;
        const uint32_t flags = (at == 0 ? CHUNK_START : 0u) | (end ? CHUNK_END : 0u) | (end && nchunks == 1 ? ROOT : 0u);
        s.compress(chunk, last ? nslots * 8 - blk * 64 : 64u, flags);
        if (end && nchunks > 1) {
            #pragma unroll
            for (int k = 0; k < MAXCHUNKS; k++)
                if (chunk == (unsigned)k) {
                    #pragma unroll
                    for (int q = 0; q < 8; q++) c[k][q] = s.cv[q];
                }
            s.init();
        }
    }
    for (unsigned p = 0; p + 1 < nchunks; p++) {
        const bool low = p == 0, pair = p == 1 && nchunks == 4;          // (c0, c1) / (c2, c3); otherwise (c0, c2)
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            s.m[q] = pair ? c[2][q] : c[0][q];
            s.m[8 + q] = low ? c[1][q] : pair ? c[3][q] : c[2][q];
        }
        s.init();
        s.compress(0, 64, PARENT | (p + 2 == nchunks ? ROOT : 0u));
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            if (pair) c[2][q] = s.cv[q];
            else c[0][q] = s.cv[q];
        }
    }
    s.put(P.leaves + r * 32);
}

// nodes[out0 + i] = H(src[2i] || src[2i+1]) for i < count; digests are 32 raw bytes
static __global__ void __launch_bounds__(NT) blake3_merge_level(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t count) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    B3 s;
    s.merge((const uint4*)(src + i * 64));
    s.put(dst + i * 32);
}

// The upper levels of a tree in few launches, as blake2s_merkle_top: workgroup b takes the NT parents [b NT, b NT + NT) of a level of
// `count` parents (count = NT: the top of the tree; count = k NT: k subtrees at once; count < NT: the tree's last levels), keeps the
// current level in LDS and climbs to ONE node, writing every level to its slot of nodes[].  PER = 2: a lane computes two adjacent
// parents and their parent in registers (half the workgroups for the widest of these levels).
template <int PER>
static __global__ void __launch_bounds__(NT) blake3_merkle_top(const uint8_t* __restrict__ src, uint8_t* __restrict__ nodes, unsigned count) {
    __shared__ uint32_t lvl[2][NT * 8];
    const unsigned t = threadIdx.x, b = blockIdx.x;
    if (count <= (unsigned)NT && b == 0 && t < 8) ((uint32_t*)nodes)[t] = 0;     // the launch that ends in the root clears nodes[0]
    unsigned mine = count < (unsigned)NT ? count : (unsigned)NT;
    size_t level = count;
    B3 s;
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
        for (int q = 0; q < 8; q++) left[q] = s.cv[q];
        s.merge(second);
        s.put(nodes + (level + n0 + 1) * 32);
        #pragma unroll
        for (int q = 0; q < 8; q++) { s.m[8 + q] = s.cv[q]; s.m[q] = left[q]; }
        level >>= 1;
        s.init();
        s.compress(0, 64, ONE_BLOCK);
    } else if (t < mine) {
        s.merge((const uint4*)(src + ((size_t)b * NT + t) * 64));
    }
    int cur = 0;
    for (;;) {
        if (t < mine) {
            s.put(nodes + (level + (size_t)b * mine + t) * 32);
            #pragma unroll
            for (int q = 0; q < 8; q++) lvl[cur][t * 8 + q] = s.cv[q];
        }
        if (mine == 1) break;
        __syncthreads();
        mine >>= 1; level >>= 1;
        if (t < mine) {
            #pragma unroll
            for (int q = 0; q < 16; q++) s.m[q] = lvl[cur][t * 16 + q];
            s.init();
            s.compress(0, 64, ONE_BLOCK);
        }
        cur ^= 1;
    }
}

// Proof-of-work (PublicCoin::grind_proof_of_work, src/random.rs:48-55, 129-132, 180-192): the smallest nonce >= 1 with
// leading_zeros(H(seed || nonce.to_be_bytes())) >= bits.  One nonce per lane over [base, base + count); the minimum hit is kept with
// atomicMin.  seed[] holds the 32 seed bytes as little-endian words (wave-uniform).
using PowParams = msb2s::PowParams;
static __global__ void __launch_bounds__(NT) blake3_pow_grind(PowParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * NT + threadIdx.x;
    if (i >= P.count) return;
    const unsigned long long nonce = P.base + i;
    B3 s;
    s.init();
    #pragma unroll
    for (int q = 0; q < 8; q++) s.m[q] = P.seed[q];
    s.m[8] = __builtin_bswap32((uint32_t)(nonce >> 32)); s.m[9] = __builtin_bswap32((uint32_t)nonce);   // big-endian u64 bytes
    #pragma unroll
    for (int q = 10; q < 16; q++) s.m[q] = 0;
    s.compress(0, 40, ONE_BLOCK);
    // mshash::leading_zero_bits<false>(s.cv), written out, as in blake2s_pow_grind
    unsigned lz = 0;
    bool done = false;
    #pragma unroll
    for (int q = 0; q < 8; q++) {
        if (!done) {
            const uint32_t w = __builtin_bswap32(s.cv[q]);
            const unsigned z = w ? (unsigned)__clz(w) : 32u;
            lz += z;
            if (z != 32) done = true;
        }
    }
    if (lz >= P.bits) atomicMin(P.found, nonce);
}

}  // namespace msb3
