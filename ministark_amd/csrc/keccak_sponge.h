// The Keccak sponge of keccak_kernels.h as device functions only -- the permutation, the one-block loaders and the digest -- for the
// units that hash inside their own kernels (coin_kernels.h) without the commitment kernels.  The rules and the instruction counts are
// stated at the top of keccak_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mskec {

static constexpr int RATE_SLOTS = 17;                         // 136 bytes
static constexpr uint32_t DOMAIN_KECCAK = 0x01u, DOMAIN_SHA3 = 0x06u;

// rho's rotation of lane x + 5 y
static constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

// iota's round constant.  With the rounds fully unrolled (permute<24>) r is a constant and the call folds to one literal per half.  In
// permute<U>, U < 24, r depends on the loop counter, which is wave-uniform: hipcc lowers the switch to a tree of scalar compares and
// branches (s_cmp / s_cbranch_scc) that ends in s_mov_b32 literals -- about five scalar instructions per round, no table in memory, no
// load.  (Checked in the listing of coin_step<3, *>; an s_load from a constant table would be the other legal lowering.)
__device__ __forceinline__ uint64_t round_constant(int r) {
    switch (r) {
        case 0: return 0x0000000000000001ull;  case 1: return 0x0000000000008082ull;  case 2: return 0x800000000000808Aull;
        case 3: return 0x8000000080008000ull;  case 4: return 0x000000000000808Bull;  case 5: return 0x0000000080000001ull;
        case 6: return 0x8000000080008081ull;  case 7: return 0x8000000000008009ull;  case 8: return 0x000000000000008Aull;
        case 9: return 0x0000000000000088ull;  case 10: return 0x0000000080008009ull; case 11: return 0x000000008000000Aull;
        case 12: return 0x000000008000808Bull; case 13: return 0x800000000000008Bull; case 14: return 0x8000000000008089ull;
        case 15: return 0x8000000000008003ull; case 16: return 0x8000000000008002ull; case 17: return 0x8000000000000080ull;
        case 18: return 0x000000000000800Aull; case 19: return 0x800000008000000Aull; case 20: return 0x8000000080008081ull;
        case 21: return 0x8000000000008080ull; case 22: return 0x0000000080000001ull; default: return 0x8000000080008008ull;
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t chi(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xD2); }   // a ^ (~b & c)
// the low word of {hi, lo} >> s, 0 < s < 32: v_alignbit_b32
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, int s) { return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)s); }
#else
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
__device__ __forceinline__ uint32_t chi(uint32_t a, uint32_t b, uint32_t c) { return a ^ (~b & c); }
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, int s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> s); }
#endif

// (ol, oh) = rotl64((l, h), n), n a compile-time constant after unrolling
__device__ __forceinline__ void rotl64(uint32_t l, uint32_t h, int n, uint32_t& ol, uint32_t& oh) {
    if (n == 0) { ol = l; oh = h; }
    else if (n == 32) { ol = h; oh = l; }
    else if (n < 32) { oh = funnel(h, l, 32 - n); ol = funnel(l, h, 32 - n); }
    else { oh = funnel(l, h, 64 - n); ol = funnel(h, l, 64 - n); }
}

struct Keccak {
    uint32_t lo[25], hi[25];                                  // lane x + 5 y of the state, as halves

    __device__ __forceinline__ void clear() {
        #pragma unroll
        for (int i = 0; i < 25; i++) { lo[i] = 0; hi[i] = 0; }
    }
    __device__ __forceinline__ void round(uint64_t rc) {
        uint32_t cl[5], ch[5], rl[5], rh[5];
        #pragma unroll
        for (int x = 0; x < 5; x++) {
            cl[x] = xor3(xor3(lo[x], lo[x + 5], lo[x + 10]), lo[x + 15], lo[x + 20]);
            ch[x] = xor3(xor3(hi[x], hi[x + 5], hi[x + 10]), hi[x + 15], hi[x + 20]);
        }
        #pragma unroll
        for (int x = 0; x < 5; x++) rotl64(cl[x], ch[x], 1, rl[x], rh[x]);
        uint32_t bl[25], bh[25];
        #pragma unroll
        for (int y = 0; y < 5; y++) {
            #pragma unroll
            for (int x = 0; x < 5; x++) {
                const uint32_t tl = xor3(lo[x + 5 * y], cl[(x + 4) % 5], rl[(x + 1) % 5]);
                const uint32_t th = xor3(hi[x + 5 * y], ch[(x + 4) % 5], rh[(x + 1) % 5]);
                const int to = y + 5 * ((2 * x + 3 * y) % 5);            // pi: B[y][2x + 3y] = rotl(A[x][y], rho)
                rotl64(tl, th, RHO[x + 5 * y], bl[to], bh[to]);
            }
        }
        #pragma unroll
        for (int y = 0; y < 5; y++) {
            #pragma unroll
            for (int x = 0; x < 5; x++) {
                lo[x + 5 * y] = chi(bl[x + 5 * y], bl[(x + 1) % 5 + 5 * y], bl[(x + 2) % 5 + 5 * y]);
                hi[x + 5 * y] = chi(bh[x + 5 * y], bh[(x + 1) % 5 + 5 * y], bh[(x + 2) % 5 + 5 * y]);
            }
        }
        lo[0] ^= (uint32_t)rc; hi[0] ^= (uint32_t)(rc >> 32);
    }
    // Keccak-f[1600] with U rounds per loop trip (U divides 24; U = 24: straight-line code, the round constants are literals)
    template <int U>
    __device__ __forceinline__ void permute() {
        #pragma unroll 1
        for (int r0 = 0; r0 < 24; r0 += U) {
            #pragma unroll
            for (int j = 0; j < U; j++) round(round_constant(r0 + j));
        }
    }
    // state = the one padded block of a message of 8 * nwords8 <= 64 bytes held in m[] (little-endian words, zero past its end)
    __device__ __forceinline__ void load_short(const uint32_t (&m)[16], unsigned nwords8, uint32_t domain) {
        clear();
        #pragma unroll
        for (int q = 0; q < 8; q++) { lo[q] = m[2 * q]; hi[q] = m[2 * q + 1]; }
        #pragma unroll
        for (int q = 1; q < 9; q++) if ((unsigned)q == nwords8) lo[q] ^= domain;
        hi[16] = 0x80000000u;
    }
    // H(64 bytes at p): the Merkle merge
    template <int U>
    __device__ __forceinline__ void merge(const uint4* __restrict__ p, uint32_t domain) {
        clear();
        #pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 x = p[q];
            lo[2 * q] = x.x; hi[2 * q] = x.y; lo[2 * q + 1] = x.z; hi[2 * q + 1] = x.w;
        }
        lo[8] = domain; hi[16] = 0x80000000u;
        permute<U>();
    }
    __device__ __forceinline__ void digest(uint32_t (&d)[8]) const {
        #pragma unroll
        for (int q = 0; q < 4; q++) { d[2 * q] = lo[q]; d[2 * q + 1] = hi[q]; }
    }
    __device__ __forceinline__ void put(uint8_t* out) const {
        uint4* o = (uint4*)out;
        o[0] = make_uint4(lo[0], hi[0], lo[1], hi[1]);
        o[1] = make_uint4(lo[2], hi[2], lo[3], hi[3]);
    }
};

// the unroll depth of the wide kernels (rows, merge level, LDS top, proof-of-work) and of the single-wave coin chains
static constexpr int UNROLL_WIDE = 24, UNROLL_CHAIN = 2;

}  // namespace mskec
