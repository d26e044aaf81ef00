// Keccak-256 and SHA3-256 Merkle commitments and proof-of-work for gfx950: the choice of H in MatrixMerkleTreeImpl<H>
// (src/merkle.rs:296-361, 412-508) and PublicCoinImpl<F, H> (src/random.rs:48-58, 61-141) that an EVM verifier recomputes with one
// opcode, through the reference's HashFn / ElementHashFn seam (src/hash.rs:9-41).  H = the Keccak sponge with rate 136 bytes,
// capacity 512 bits and a 32-byte digest; the two members differ in ONE byte, the domain byte appended to the message:
//   Keccak-256  0x01  the original submission's padding (sha3::Keccak256, the EVM's KECCAK256)
//   SHA3-256    0x06  FIPS 202 (sha3::Sha3_256, hashlib.sha3_256)
// so one kernel set serves both and the byte is a wave-uniform launch argument.
//   leaf[r]   = H( ||_c canonical little-endian bytes of M[c][r] )   -- the bytes ms_sha256_rows / ms_blake2s_rows hash
//               (Fp: 8 bytes, Fq3: c0||c1||c2, Fp252: 32 bytes); a row of L bytes is floor(L / 136) + 1 blocks
//   nodes[k]  = H(nodes[2k] || nodes[2k+1]): 64 bytes, ONE permutation
//   pow       = H(seed32 || nonce as 8 big-endian bytes): 40 bytes, one permutation
// Padding: the domain byte at offset L mod 136 of the last block, 0x80 ORed into that block's byte 135; L = 0 mod 136 gives one more
// block that holds only padding.  Every message here is a whole number of 8-byte slots (17 per block), so the domain byte is byte 0 of
// slot L / 8 mod 17 and 0x80 byte 7 of slot 16 -- two word XORs, no byte-granular padder (L = 128 mod 136: both in slot 16).  Lanes are
// little-endian, so canonical limbs and digests go in and out of the state without byte swaps.  The digest is lanes 0..3.
//
// Keccak-f[1600]: 25 lanes of 64 bits as 50 32-bit registers, 24 rounds, per round
//   theta  C[x] = the five-way column XOR, two three-input XORs per half (v_bitop3_b32 0x96); D[x] = C[x-1] ^ rotl(C[x+1], 1) is never
//          formed: A ^ D is one more three-input XOR per half with the rotated column
//   rho    rotl64 by a constant: two v_alignbit_b32 (a register swap when the amount is 32 -- none of Keccak's 24 amounts is)
//   pi     register renaming: B[y][2x+3y] = rotl(A[x][y]), indices resolved at compile time
//   chi    a ^ (~b & c): one v_bitop3_b32 (0xD2) per half
//   iota   a literal per half when the rounds are fully unrolled (permute<24>); permute<U>, U < 24, keeps a loop of 24 / U trips
//          and selects the constant by scalar branches on the loop counter (still literals, no load: keccak_sponge.h)
// = 20 + 10 + 50 + 48 + 50 + 2 = 180 vector instructions per round.  Layout and launch shapes are those of blake2s_kernels.h: one
// row (or node) per lane, column reads coalesced, the top of a tree climbed in LDS by one workgroup per subtree.  The sponge itself
// (permutation, one-block loaders, digest) is keccak_sponge.h, which coin_kernels.h includes without these kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "gl.h"
#include "gl_dev.h"
#include "fp252.h"
#include "keccak_sponge.h"
#include "hash_dev.h"

namespace mskec {

static constexpr int MAXCOLS = 128;
static constexpr int NT = 256;

struct RowsParams {
    const uint64_t* cols[MAXCOLS];
    uint8_t* leaves;          // nrows x 32 bytes
    size_t nrows;
    unsigned ncols;
    unsigned row_stride;      // words between consecutive rows of one column (V when columns are dense)
    uint32_t domain;          // 0x01 Keccak-256, 0x06 SHA3-256
};

// slots j = 0..16 of a block from the limb sequence W: slot j is W[4 - F + j], F = the slot at which the block's first new element starts
template <int F>
__device__ __forceinline__ void absorb_limbs(Keccak& s, const uint64_t (&W)[24]) {
    #pragma unroll
    for (int j = 0; j < RATE_SLOTS; j++) { s.lo[j] ^= (uint32_t)W[4 - F + j]; s.hi[j] ^= (uint32_t)(W[4 - F + j] >> 32); }
}

// One row per lane; V = u64 words per element (1 Fp, 3 Fq3, 4 Fp252).  The message is a stream of 8-byte slots: slot i < nslots is
// limb (i % V) of the element of column i / V as its canonical value.  A block is 17 slots, XORed into lanes 0..16 with compile-time
// register indices; 17 is a multiple of neither 3 nor 4, so elements straddle blocks.  Fp and Fq3 limbs convert one by one.  A 252-bit
// element converts as a whole, so the element that straddles the end of a block is carried to the next one: block blk starts at limb
// blk & 3 of an element (17 = 1 mod 4), its new elements start at slots F, F + 4, ..., F = (4 - blk) & 3, and with the carried element
// in front the block is 17 consecutive entries of one limb sequence, taken at an offset that depends on F alone.
template <int V>
static __global__ void __launch_bounds__(NT) keccak_rows(RowsParams P) {
    const size_t r = (size_t)blockIdx.x * NT + threadIdx.x;
    if (r >= P.nrows) return;
    Keccak s;
    s.clear();
    const unsigned nslots = P.ncols * V;
    const unsigned nblocks = nslots / RATE_SLOTS + 1;
    f252::E carried = f252::zero();
    for (unsigned blk = 0; blk < nblocks; blk++) {
        if constexpr (V == 4) {
            const unsigned first = (4 - (blk & 3)) & 3;
            const unsigned e0 = (blk * RATE_SLOTS + first) / 4;              // the first element that starts in this block
            uint64_t W[24];
            #pragma unroll
            for (int q = 0; q < 4; q++) W[q] = carried.l[q];
            #pragma unroll
            for (int k = 0; k < 5; k++) {                                    // the fifth starts in this block only when first = 0 (slot 16)
                f252::E t = f252::zero();
                if (e0 + k < P.ncols && (k < 4 || first == 0)) {
                    const uint64_t* __restrict__ e = P.cols[e0 + k] + r * P.row_stride;
                    t = f252::from_mont(f252::E{{e[0], e[1], e[2], e[3]}});
                    carried = t;
                }
                #pragma unroll
                for (int q = 0; q < 4; q++) W[4 + 4 * k + q] = t.l[q];
            }
            if (first == 0) absorb_limbs<0>(s, W);
            else if (first == 1) absorb_limbs<1>(s, W);
            else if (first == 2) absorb_limbs<2>(s, W);
            else absorb_limbs<3>(s, W);
        } else {
            #pragma unroll
            for (int j = 0; j < RATE_SLOTS; j++) {
                const unsigned i = blk * RATE_SLOTS + j;
                if (i < nslots) {
                    const unsigned c = i / V, v = i - c * V;
                    const uint64_t* __restrict__ e = P.cols[c] + r * P.row_stride;
                    const uint64_t x = gld::mmul(e[v], 1);                   // out of Montgomery form, canonical
                    s.lo[j] ^= (uint32_t)x; s.hi[j] ^= (uint32_t)(x >> 32);
                }
            }
        }
        const unsigned pad = nslots - blk * RATE_SLOTS;                      // < 17 in the last block only
        #pragma unroll
        for (int j = 0; j < RATE_SLOTS; j++) if ((unsigned)j == pad) s.lo[j] ^= P.domain;
        if (blk + 1 == nblocks) s.hi[16] ^= 0x80000000u;
        s.permute<UNROLL_WIDE>();
    }
    s.put(P.leaves + r * 32);
}

// nodes[out0 + i] = H(src[2i] || src[2i+1]) for i < count; digests are 32 raw bytes
static __global__ void __launch_bounds__(NT) keccak_merge_level(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t count, uint32_t domain) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    Keccak s;
    s.merge<UNROLL_WIDE>((const uint4*)(src + i * 64), domain);
    s.put(dst + i * 32);
}

// The upper levels of a tree in few launches, as blake2s_merkle_top: workgroup b takes the NT parents [b NT, b NT + NT) of a level of
// `count` parents (count = NT: the top of the tree; count = k NT: k subtrees at once; count < NT: the tree's last levels), keeps the
// current level in LDS and climbs to ONE node, writing every level to its slot of nodes[].  PER = 2: a lane computes two adjacent
// parents and their parent first (half the workgroups for the widest of these levels).  Every merge goes through the one loop below, so
// the kernel holds a single copy of the permutation: `msg` is the lane's next 64-byte message.
template <int PER>
static __global__ void __launch_bounds__(NT) keccak_merkle_top(const uint8_t* __restrict__ src, uint8_t* __restrict__ nodes, unsigned count, uint32_t domain) {
    __shared__ __attribute__((aligned(16))) uint32_t lvl[2][NT * 8];      // read back 64 bytes per lane as four uint4
    const unsigned t = threadIdx.x, b = blockIdx.x;
    if (count <= (unsigned)NT && b == 0 && t < 8) ((uint32_t*)nodes)[t] = 0;     // the launch that ends in the root clears nodes[0]
    unsigned mine = count < (unsigned)NT ? count : (unsigned)NT;
    size_t level = count;
    Keccak s;
    uint4 msg[4];
    int pre = 0;                                                          // PER = 2: 0 and 1 are the lane's two parents, 2 is their parent
    uint32_t left[8];
    const size_t n0 = PER == 2 ? (size_t)b * 2 * NT + 2 * t : (size_t)b * NT + t;   // PER = 2: count is a multiple of 2 NT
    if (PER == 2 || t < mine) {
        const uint4* in = (const uint4*)(src + n0 * 64);
        #pragma unroll
        for (int q = 0; q < 4; q++) msg[q] = in[q];
    }
    int cur = 0;
    for (;;) {
        if (PER == 2 || t < mine) s.merge<UNROLL_WIDE>(msg, domain);
        if (PER == 2 && pre < 2) {
            s.put(nodes + (level + n0 + pre) * 32);
            if (pre == 0) {
                s.digest(left);
                const uint4* in = (const uint4*)(src + (n0 + 1) * 64);
                #pragma unroll
                for (int q = 0; q < 4; q++) msg[q] = in[q];
            } else {
                msg[0] = make_uint4(left[0], left[1], left[2], left[3]); msg[1] = make_uint4(left[4], left[5], left[6], left[7]);
                msg[2] = make_uint4(s.lo[0], s.hi[0], s.lo[1], s.hi[1]); msg[3] = make_uint4(s.lo[2], s.hi[2], s.lo[3], s.hi[3]);
                level >>= 1;
            }
            pre++;
            continue;
        }
        if (t < mine) {
            uint32_t d[8];
            s.digest(d);
            s.put(nodes + (level + (size_t)b * mine + t) * 32);
            #pragma unroll
            for (int q = 0; q < 8; q++) lvl[cur][t * 8 + q] = d[q];
        }
        if (mine == 1) break;
        __syncthreads();
        mine >>= 1; level >>= 1;
        if (t < mine) {
            const uint4* in = (const uint4*)&lvl[cur][t * 16];
            #pragma unroll
            for (int q = 0; q < 4; q++) msg[q] = in[q];
        }
        cur ^= 1;
    }
}

// Proof-of-work (PublicCoin::grind_proof_of_work, src/random.rs:48-58): the smallest nonce >= 1 with
// leading_zeros(H(seed || nonce.to_be_bytes())) >= bits.  One nonce per lane over [base, base + count); the minimum hit is kept with
// atomicMin.  seed[] holds the 32 seed bytes as little-endian words (wave-uniform).
struct PowParams { uint32_t seed[8]; unsigned long long base; unsigned long long count; unsigned bits; uint32_t domain; unsigned long long* found; };

static __global__ void __launch_bounds__(NT) keccak_pow_grind(PowParams P) {
    const unsigned long long i = (unsigned long long)blockIdx.x * NT + threadIdx.x;
    if (i >= P.count) return;
    const unsigned long long nonce = P.base + i;
    uint32_t m[16];
    #pragma unroll
    for (int q = 0; q < 8; q++) m[q] = P.seed[q];
    m[8] = __builtin_bswap32((uint32_t)(nonce >> 32)); m[9] = __builtin_bswap32((uint32_t)nonce);   // big-endian u64 bytes
    #pragma unroll
    for (int q = 10; q < 16; q++) m[q] = 0;
    Keccak s;
    s.load_short(m, 5, P.domain);
    s.permute<UNROLL_WIDE>();
    uint32_t d[8];
    s.digest(d);
    if (mshash::leading_zero_bits<false>(d) >= P.bits) atomicMin(P.found, nonce);
}

}  // namespace mskec
